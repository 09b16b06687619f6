// The small kernels of the perceptual-loss plans (lpips_ops.hip holds their host dispatch, lpips.py the planner):
//   SF_OP_POOL   2x2 max pooling, forward and backward
//   SF_OP_LPIPS  per-layer head: channel-unit-normalise both feature maps, squared difference, non-negative
//                1x1 "lin" weights, spatial mean -- forward (scalar per sample) and backward (d / d features of
//                the first image; the second image is the no-grad target)
//   eltwise helpers: ReLU backward, the input scaling layer and its gradient
// All of it is elementwise / per-pixel reductions in fp32: HBM bound, one wave per pixel for the head.
// Written against sf_dev.h so that tests/hostemu/lpips_emu.cpp runs this source on CPU fibers; lpips_launch_of() below is the op
// decoding both the gfx950 dispatch and that harness launch from.
#pragma once
#include "sf_dev.h"
#include "../../include/sparsefusion_hip.h"

// ---- max pooling -------------------------------------------------------------------------------------------
SF_KERNEL(256) void k_pool_fwd(const float* __restrict__ in, float* __restrict__ out, int B, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, c4 = C / 4;
  const long total = (long)B * Ho * Wo * c4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % c4) * 4;
    long r = i / c4;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const float* p = in + (((long)b * H + 2 * oy) * W + 2 * ox) * C + c;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), bq = *reinterpret_cast<const f32x4*>(p + C);
    const f32x4 cq = *reinterpret_cast<const f32x4*>(p + (long)W * C), d = *reinterpret_cast<const f32x4*>(p + (long)W * C + C);
    f32x4 m;
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = fmaxf(fmaxf(a[j], bq[j]), fmaxf(cq[j], d[j]));
    *reinterpret_cast<f32x4*>(out + (((long)b * Ho + oy) * Wo + ox) * C + c) = m;
  }
}

// din gets dout at the FIRST window position (row-major) that holds the maximum, 0 elsewhere (torch's argmax rule)
SF_KERNEL(256) void k_pool_bwd(const float* __restrict__ dout, const float* __restrict__ in, float* __restrict__ din, int B, int H,
                               int W, int C) {
  const int Ho = H / 2, Wo = W / 2, c4 = C / 4;
  const long total = (long)B * Ho * Wo * c4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % c4) * 4;
    long r = i / c4;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const long base = (((long)b * H + 2 * oy) * W + 2 * ox) * C + c;
    const long offs[4] = {0, C, (long)W * C, (long)W * C + C};
    f32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const f32x4*>(in + base + offs[k]);
    const f32x4 g = *reinterpret_cast<const f32x4*>(dout + (((long)b * Ho + oy) * Wo + ox) * C + c);
    f32x4 o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int arg = 0;
      float m = v[0][j];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (v[k][j] > m) { m = v[k][j]; arg = k; }
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k][j] = (k == arg) ? g[j] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4*>(din + base + offs[k]) = o[k];
  }
}

// ---- LPIPS head ---------------------------------------------------------------------------------------------
// feats [2V, HW, C]: samples 0..V-1 = in0 (gradient flows), V..2V-1 = in1.  One wave per pixel.
//   u = f0 / (|f0| + eps), v = f1 / (|f1| + eps), d = sum_c w_c (u_c - v_c)^2, acc[s] += mean_pixels d
// The workgroups of all five layers meet in acc[s]: a 2^-44 fixed-point integer (SF_FIX_ONE, sf_dev.h: a distance is O(1), a workgroup's
// share of it is kept to 6e-14), so that the sum does not depend on the order in which they arrive (an fp32 atomic here made the
// distance, and every loss built on it, differ in its last bits from run to run); k_lpips_head_sum turns it into the float the caller reads.
#define LPIPS_EPS 1e-10f
SF_KERNEL(256) void k_lpips_head_fwd(const float* __restrict__ feats, const float* __restrict__ w, long long* __restrict__ out, int V,
                                     int HW, int C) {
  SF_SHARED float red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int per_sample_blocks = gridDim.x / V;
  const int s = blockIdx.x / per_sample_blocks, bl = blockIdx.x % per_sample_blocks;
  float acc = 0.0f;
  for (int p = bl * 4 + wv; p < HW; p += per_sample_blocks * 4) {
    const float* f0 = feats + ((long)s * HW + p) * C;
    const float* f1 = feats + ((long)(V + s) * HW + p) * C;
    float n0 = 0.0f, n1 = 0.0f;
    for (int c = lane * 4; c < C; c += 256) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(f0 + c), b = *reinterpret_cast<const f32x4*>(f1 + c);
      n0 += a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3];
      n1 += b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3];
    }
    n0 = sf_wave_sum(n0); n1 = sf_wave_sum(n1);
    const float r0 = 1.0f / (sqrtf(n0) + LPIPS_EPS), r1 = 1.0f / (sqrtf(n1) + LPIPS_EPS);
    float d = 0.0f;
    for (int c = lane * 4; c < C; c += 256) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(f0 + c), b = *reinterpret_cast<const f32x4*>(f1 + c);
      const f32x4 ww = *reinterpret_cast<const f32x4*>(w + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = a[j] * r0 - b[j] * r1;
        d = fmaf(ww[j] * e, e, d);
      }
    }
    acc += sf_wave_sum(d);
  }
  if (lane == 0) red[wv] = acc;
  sf_sync();
  if (threadIdx.x == 0) {
    const float part = (red[0] + red[1] + red[2] + red[3]) / (float)HW;
    sf_fix_add(out + s, sf_fix_of(part));
  }
}

SF_KERNEL(64) void k_lpips_head_sum(const long long* __restrict__ acc, float* __restrict__ out, int V) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s < V) out[s] = (float)((double)acc[s] * (1.0 / SF_FIX_ONE));
}

// dfeat[s, p, :] = gscale[s] / HW * d d_p / d f0:  a_c = 2 w_c (u_c - v_c);  df = a / n - f0 * (a . f0) / (n^2 |f0|)
// (a pixel whose f0 is all zero: k2 = 0, i.e. the one-sided limit g / HW * 2 w (0 - v) / (0 + eps))
SF_KERNEL(256) void k_lpips_head_bwd(const float* __restrict__ feats, const float* __restrict__ w, const float* __restrict__ gscale,
                                     float* __restrict__ dfeat, int V, int HW, int C) {
  const int lane = threadIdx.x & 63;
  const long pixels = (long)V * HW;
  for (long q = blockIdx.x * 4L + (threadIdx.x >> 6); q < pixels; q += (long)gridDim.x * 4) {
    const int s = (int)(q / HW);
    const float* f0 = feats + q * C;
    const float* f1 = feats + ((long)V * HW + q) * C;
    float n0 = 0.0f, n1 = 0.0f;
    for (int c = lane * 4; c < C; c += 256) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(f0 + c), b = *reinterpret_cast<const f32x4*>(f1 + c);
      n0 += a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3];
      n1 += b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3];
    }
    n0 = sf_wave_sum(n0); n1 = sf_wave_sum(n1);
    const float l0 = sqrtf(n0);
    const float r0 = 1.0f / (l0 + LPIPS_EPS), r1 = 1.0f / (sqrtf(n1) + LPIPS_EPS);
    float dot = 0.0f;
    for (int c = lane * 4; c < C; c += 256) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(f0 + c), b = *reinterpret_cast<const f32x4*>(f1 + c);
      const f32x4 ww = *reinterpret_cast<const f32x4*>(w + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) dot = fmaf(2.0f * ww[j] * (a[j] * r0 - b[j] * r1), a[j], dot);
    }
    dot = sf_wave_sum(dot);
    const float g = gscale[s] / (float)HW;
    const float k2 = l0 > 0.0f ? dot * r0 * r0 / l0 : 0.0f;
    for (int c = lane * 4; c < C; c += 256) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(f0 + c), b = *reinterpret_cast<const f32x4*>(f1 + c);
      const f32x4 ww = *reinterpret_cast<const f32x4*>(w + c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = g * (2.0f * ww[j] * (a[j] * r0 - b[j] * r1) * r0 - a[j] * k2);
      *reinterpret_cast<f32x4*>(dfeat + q * C + c) = o;
    }
  }
}

// ---- elementwise helpers ------------------------------------------------------------------------------------
// out (operand type) = dy * (y > 0)      (ReLU backward; y is the post-ReLU activation)
SF_KERNEL(256) void k_relu_bwd(const float* __restrict__ dy, const float* __restrict__ y, sf_opnd* __restrict__ out, long n4) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(dy + i * 4), a = *reinterpret_cast<const f32x4*>(y + i * 4);
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (sf_opnd)(a[j] > 0.0f ? g[j] : 0.0f);
    *reinterpret_cast<bf16x4*>(out + i * 4) = o;
  }
}

// ScalingLayer: out NHWC [B, HW, Cp] (zero padded) = (x NCHW [B, 3, HW] - shift[c]) / scale[c] ; k = (shift3, scale3)
SF_KERNEL(256) void k_scale_in(const float* __restrict__ x, const float* __restrict__ k, float* __restrict__ out, int B, int HW, int Cp) {
  const long n = (long)B * HW * Cp;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = (int)(i % Cp);
    const long bp = i / Cp;
    const int p = (int)(bp % HW), b = (int)(bp / HW);
    out[i] = c < 3 ? (x[((long)b * 3 + c) * HW + p] - k[c]) / k[3 + c] : 0.0f;
  }
}
// its gradient: dx NCHW [B, 3, HW] = g NHWC [B, HW, ld][.., c] / scale[c]
SF_KERNEL(256) void k_scale_in_bwd(const float* __restrict__ g, const float* __restrict__ k, float* __restrict__ dx, int B, int HW,
                                   int ld) {
  const long n = (long)B * 3 * HW;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long bc = i / HW;
    const int c = (int)(bc % 3), b = (int)(bc / 3);
    dx[i] = g[((long)b * HW + p) * ld + c] / k[3 + c];
  }
}

// ---- op decoding: which kernel, how many workgroups ------------------------------------------------------------
enum LpipsKernel { LP_POOL_FWD = 1, LP_POOL_BWD, LP_HEAD_FWD, LP_HEAD_SUM, LP_HEAD_BWD, LP_RELU_BWD, LP_SCALE_IN, LP_SCALE_IN_BWD };
struct LpipsLaunch { int kernel; uint32_t grid, block; const char* name; };

// workgroups of a grid-stride launch over `work` items, `per` items per workgroup: enough to fill the chip (256 CUs x 8 resident 256-thread blocks)
static inline uint32_t lpips_grid(uint64_t work, uint64_t per) {
  const uint64_t want = (uint32_t)((work + per - 1) / per), cap = 256ull * 8ull;
  return (uint32_t)(want < cap ? (want ? want : 1) : cap);
}

// The launch of a SF_OP_POOL (flags 0 / 1) / SF_OP_LPIPS / SF_OP_ELTWISE (7 / 8 / 9) op; returns the error text of a bad op, else NULL.
static inline const char* lpips_launch_of(const sf_op& op, LpipsLaunch& L) {
  L.block = 256;
  switch (op.type) {
    case SF_OP_POOL: {
      const int B = op.i[0], H = op.i[1], W = op.i[2], C = op.i[3];
      if ((H | W) & 1 || C % 4) return "pool: H, W must be even and C a multiple of 4";
      L.grid = lpips_grid((uint64_t)((long)B * (H / 2) * (W / 2) * (C / 4)), 256);
      L.name = "pool";
      if (op.flags == 0) {
        if (!op.p[0] || !op.p[3]) return "pool: null tensor";
        L.kernel = LP_POOL_FWD;
      } else {
        if (!op.p[0] || !op.p[1] || !op.p[3]) return "pool backward: null tensor";
        L.kernel = LP_POOL_BWD;
      }
      return nullptr;
    }
    case SF_OP_LPIPS: {
      const int V = op.i[0], HW = op.i[1], C = op.i[2];
      if (op.flags == 2) {                                   // the accumulated distances p[2] (fixed point) -> p[3] (float)
        if (V < 1 || !op.p[2] || !op.p[3] || ((uintptr_t)op.p[2] & 7)) return "lpips head sum: bad operands";
        L.kernel = LP_HEAD_SUM; L.grid = (uint32_t)(((uint64_t)V + 63) / 64); L.block = 64; L.name = "lpips_head_sum";
        return nullptr;
      }
      if (V < 1 || C % 4 || !op.p[0] || !op.p[1] || !op.p[3]) return "lpips head: bad operands";
      L.name = "lpips_head";
      if (op.flags == 0) {
        if ((uintptr_t)op.p[3] & 7) return "lpips head: the accumulator is a 64-bit integer per sample";
        int per = (int)(((uint64_t)HW + 3) / 4);
        if (per > 256) per = 256;                            // one atomic per workgroup: keep them few
        L.kernel = LP_HEAD_FWD; L.grid = (uint32_t)(V * per);
      } else {
        if (!op.p[2]) return "lpips head backward: missing upstream gradient";
        L.kernel = LP_HEAD_BWD; L.grid = lpips_grid((uint64_t)V * HW, 4);
      }
      return nullptr;
    }
    case SF_OP_ELTWISE:
      L.name = "eltwise";
      switch (op.flags) {
        case 7: L.kernel = LP_RELU_BWD; L.grid = lpips_grid((uint64_t)((long)(uint32_t)op.i[0] / 4), 256); return nullptr;
        case 8: L.kernel = LP_SCALE_IN; L.grid = lpips_grid((uint64_t)((long)op.i[0] * op.i[1] * op.i[2]), 256); return nullptr;
        case 9: L.kernel = LP_SCALE_IN_BWD; L.grid = lpips_grid((uint64_t)((long)op.i[0] * 3 * op.i[1]), 256); return nullptr;
        default: return "eltwise: unknown mode";
      }
    default: return "plan: unknown op type";
  }
}

// The launch itself, once per build: LAUNCH(kernel, args...) is <<<L.grid, L.block, 0, stream>>> on gfx950 and hipemu::launch under emulation.
#define LPIPS_DISPATCH(op, L, LAUNCH)                                                                                                       \
  switch ((L).kernel) {                                                                                                                     \
    case LP_POOL_FWD: LAUNCH(k_pool_fwd, (const float*)(op).p[0], (float*)(op).p[3], (op).i[0], (op).i[1], (op).i[2], (op).i[3]); break;       \
    case LP_POOL_BWD:                                                                                                                       \
      LAUNCH(k_pool_bwd, (const float*)(op).p[0], (const float*)(op).p[1], (float*)(op).p[3], (op).i[0], (op).i[1], (op).i[2], (op).i[3]);    \
      break;                                                                                                                                \
    case LP_HEAD_FWD:                                                                                                                       \
      LAUNCH(k_lpips_head_fwd, (const float*)(op).p[0], (const float*)(op).p[1], (long long*)(op).p[3], (op).i[0], (op).i[1], (op).i[2]);     \
      break;                                                                                                                                \
    case LP_HEAD_SUM: LAUNCH(k_lpips_head_sum, (const long long*)(op).p[2], (float*)(op).p[3], (op).i[0]); break;                           \
    case LP_HEAD_BWD:                                                                                                                       \
      LAUNCH(k_lpips_head_bwd, (const float*)(op).p[0], (const float*)(op).p[1], (const float*)(op).p[2], (float*)(op).p[3], (op).i[0],       \
             (op).i[1], (op).i[2]);                                                                                                         \
      break;                                                                                                                                \
    case LP_RELU_BWD:                                                                                                                       \
      LAUNCH(k_relu_bwd, (const float*)(op).p[0], (const float*)(op).p[1], (sf_opnd*)(op).p[3], (long)(uint32_t)(op).i[0] / 4);              \
      break;                                                                                                                                \
    case LP_SCALE_IN:                                                                                                                       \
      LAUNCH(k_scale_in, (const float*)(op).p[0], (const float*)(op).p[1], (float*)(op).p[3], (op).i[0], (op).i[1], (op).i[2]);               \
      break;                                                                                                                                \
    case LP_SCALE_IN_BWD:                                                                                                                   \
      LAUNCH(k_scale_in_bwd, (const float*)(op).p[0], (const float*)(op).p[1], (float*)(op).p[3], (op).i[0], (op).i[1], (op).i[2]);           \
      break;                                                                                                                                \
    default: break;                                                                                                                         \
  }

// Camera-coverage culling of the cascaded density grid (NeRFRenderer.mark_untrained_grid, external/nerf/renderer.py:379-442): every
// cell that no camera sees gets density -1, which update_extra_state never revives and packbits never sets.  The reference walks the
// grid in a five-level Python loop with [S, 64^3, 3] temporaries per block and cascade; here it is ONE launch over the grid in storage
// (Morton) order, one lane per Morton index: the cell (x, y, z) comes from sf_compact_bits (morton3D_invert's helper) once and serves
// all C cascades, so the grid / count accesses of a wave are contiguous, as update_extra_state's are.
//
// THE TEST of one (cell, cascade, camera) triple, in float32, one rounding per operation, no contraction (SF_MUL / SF_ADD / SF_SUB /
// SF_DIV of ngp_device.h), in this order -- tests/mark_untrained_common.py restates it operation for operation:
//   w_a     = 2 * float(c_a) / float(H - 1) - 1                      a = x, y, z            (IEEE division)
//   bound_c = min(2^cas, bound),  hg = bound_c / float(H),  s = bound_c - hg,  hg2 = hg * 2
//   p_a     = w_a * s
//   q_a     = p_a - t_a                                              t = pose[:3, 3]
//   cam_j   = (q_0 * R_0j + q_1 * R_1j) + q_2 * R_2j                 R = pose[:3, :3]: cam = q @ R (pose is camera-to-world)
//   rx = cx / fx,  ry = cy / fy                                      (IEEE float32 division of the float32 intrinsics, once per camera)
//   covered = cam_2 > 0  &&  |cam_0| < rx * cam_2 + hg2  &&  |cam_1| < ry * cam_2 + hg2
// (the reference divides the Python numbers cx / fx in double and the tensor op rounds the quotient to float32: the same float32 unless
// the double quotient falls next to a float32 rounding boundary, and always when the quotient is exact; for `bound` a float32 value and
// H a power of two hg, s and hg2 are the reference's, which forms them in double.)
//
// The camera index is wave-uniform.  Read through uniform global addresses the 12 pose floats and the ratios came out as per-lane
// vector loads (the grid is written by the same kernel, so hipcc does not prove them read-only) with two IEEE divisions per wave and
// camera; so a workgroup stages OCC_MARK_CAMS cameras at a time in LDS -- pose rows and the two ratios, divided once per workgroup --
// and every lane reads them back as four broadcast 16-byte reads.  B <= OCC_MARK_CAMS: staged once, for all cascades.  With count == NULL a wave leaves the camera loop of a cascade as soon as every live lane of it is
// covered (one ballot per camera); with count it runs all B cameras and stores the number of covering cameras.  A cell with no covering
// camera gets -1 whatever it held; every other cell is left unwritten.
// n_marked: a shuffle reduction per wave, the four wave sums through LDS, ONE integer atomic per workgroup, and at most
// OCC_MARK_MAX_BLOCKS workgroups that stride over the tiles of OCC_MARK_BLOCK cells.  Atomics on one word retire at about one per
// 10 ns on gfx950 whoever issues them: with one atomic per wave of a one-tile-per-workgroup grid (32 768 at 128^3) the launch
// measured 318 us whatever B was; 2048 of them cost ~20 us, spread over the launch (profiles/mark_untrained_time.log).
// No lane returns before the end (the ballot, the shuffles and the barriers are rendezvous under tests/hostemu): lanes past H^3 idle as
// "covered".  Written against sf_dev.h so that tests/hostemu/occ_mark_emu.cpp runs this source on CPU fibers.
#pragma once
#include "sf_dev.h"
#include "ngp_device.h"

#define OCC_MARK_BLOCK 256
#define OCC_MARK_CAMS 128                // cameras staged in LDS at a time (8 KiB)
#define OCC_MARK_MAX_BLOCKS 2048          // 256 CUs x 8 workgroups: 32 waves per CU

// every third bit of x, packed (the inverse of the Morton bit spread): morton3D_invert, raymarching/src/raymarching.cu:67-82
SF_DEV uint32_t sf_compact_bits(uint32_t x) {
  x = x & 0x49249249u;
  x = (x | (x >> 2)) & 0xc30c30c3u;
  x = (x | (x >> 4)) & 0x0f00f00fu;
  x = (x | (x >> 8)) & 0xff0000ffu;
  x = (x | (x >> 16)) & 0x0000ffffu;
  return x;
}

#ifdef SF_HOST_EMU
static inline void occ_mark_add(uint32_t* p, uint32_t v) { (void)__atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#else
SF_DEV void occ_mark_add(uint32_t* p, uint32_t v) { (void)atomicAdd(p, v); }      // global_atomic_add_u32
#endif

struct OccMarkArgs {
  const float* poses;        // [B][4][4] camera-to-world, row-major
  const float* intrinsics;   // [B][4] fx fy cx cy
  uint32_t B, C, H;
  float bound;
  float* grid;               // [C][H^3], in place
  int32_t* count;            // [C][H^3] or null
  uint32_t* n_marked;        // one word, zeroed before the launch
};

// workgroups of the launch: every tile of OCC_MARK_BLOCK cells up to eight workgroups per CU, beyond that the workgroups stride over the tiles
static inline uint32_t occ_mark_grid(uint32_t H) {
  const uint64_t tiles = ((uint64_t)H * H * H + OCC_MARK_BLOCK - 1) / OCC_MARK_BLOCK;
  return (uint32_t)(tiles < OCC_MARK_MAX_BLOCKS ? tiles : OCC_MARK_MAX_BLOCKS);
}

SF_KERNEL(OCC_MARK_BLOCK) void k_occ_mark_untrained(OccMarkArgs a) {
  // a chunk of cameras, 16 floats each: rows 0..2 of the pose (R_i0 R_i1 R_i2 t_i), then cx / fx, cy / fy, 0, 0
  SF_SHARED __attribute__((aligned(16))) float cam[OCC_MARK_CAMS][16];
  SF_SHARED uint32_t wave_marked[OCC_MARK_BLOCK / 64];
  const uint32_t H3 = a.H * a.H * a.H;
  const uint32_t tiles = (H3 + OCC_MARK_BLOCK - 1) / OCC_MARK_BLOCK;
  const float hm1 = (float)(a.H - 1);
  const bool early = a.count == nullptr;
  const bool one_chunk = a.B <= OCC_MARK_CAMS;             // the chunk staged first serves every cascade of every tile
  uint32_t marked = 0;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // workgroup-uniform
    const uint32_t idx = tile * OCC_MARK_BLOCK + threadIdx.x;
    const bool live = idx < H3;
    const float w0 = SF_SUB(SF_DIV(SF_MUL(2.0f, (float)sf_compact_bits(idx)), hm1), 1.0f);
    const float w1 = SF_SUB(SF_DIV(SF_MUL(2.0f, (float)sf_compact_bits(idx >> 1)), hm1), 1.0f);
    const float w2 = SF_SUB(SF_DIV(SF_MUL(2.0f, (float)sf_compact_bits(idx >> 2)), hm1), 1.0f);
    for (uint32_t cas = 0; cas < a.C; ++cas) {
      const float bc = fminf(scalbnf(1.0f, (int)cas), a.bound);
      const float hg = SF_DIV(bc, (float)a.H);
      const float s = SF_SUB(bc, hg), hg2 = SF_MUL(hg, 2.0f);
      const float p0 = SF_MUL(w0, s), p1 = SF_MUL(w1, s), p2 = SF_MUL(w2, s);
      uint32_t n = 0;
      bool done = false;                                   // wave-uniform: every live lane of the wave is covered (early exit only)
      for (uint32_t base = 0; base < a.B; base += OCC_MARK_CAMS) {
        const uint32_t nb = a.B - base < OCC_MARK_CAMS ? a.B - base : OCC_MARK_CAMS;
        if ((tile == blockIdx.x && cas == 0) || !one_chunk) {      // workgroup-uniform: every wave meets both barriers, finished or not
          sf_sync();                                       // the previous chunk has been read by every wave
          for (uint32_t t = threadIdx.x; t < nb * 16; t += OCC_MARK_BLOCK) {
            const uint32_t j = t >> 4, k = t & 15;
            const float* K = a.intrinsics + (size_t)(base + j) * 4;
            float v = 0.0f;
            if (k < 12) v = a.poses[(size_t)(base + j) * 16 + k];
            else if (k == 12) v = SF_DIV(K[2], K[0]);
            else if (k == 13) v = SF_DIV(K[3], K[1]);
            cam[j][k] = v;
          }
          sf_sync();
        }
        for (uint32_t j = 0; j < nb && !done; ++j) {
          if (early && !sf_wave_any(live && n == 0)) { done = true; break; }
          const f32x4 r0 = *reinterpret_cast<const f32x4*>(&cam[j][0]), r1 = *reinterpret_cast<const f32x4*>(&cam[j][4]);
          const f32x4 r2 = *reinterpret_cast<const f32x4*>(&cam[j][8]), k4 = *reinterpret_cast<const f32x4*>(&cam[j][12]);
          const float q0 = SF_SUB(p0, r0[3]), q1 = SF_SUB(p1, r1[3]), q2 = SF_SUB(p2, r2[3]);
          const float cx = SF_ADD(SF_ADD(SF_MUL(q0, r0[0]), SF_MUL(q1, r1[0])), SF_MUL(q2, r2[0]));
          const float cy = SF_ADD(SF_ADD(SF_MUL(q0, r0[1]), SF_MUL(q1, r1[1])), SF_MUL(q2, r2[1]));
          const float cz = SF_ADD(SF_ADD(SF_MUL(q0, r0[2]), SF_MUL(q1, r1[2])), SF_MUL(q2, r2[2]));
          const bool in_x = fabsf(cx) < SF_ADD(SF_MUL(k4[0], cz), hg2), in_y = fabsf(cy) < SF_ADD(SF_MUL(k4[1], cz), hg2);
          n += ((cz > 0.0f) & in_x & in_y) ? 1u : 0u;
        }
      }
      if (live) {
        const size_t at = (size_t)cas * H3 + idx;
        if (a.count) a.count[at] = (int32_t)n;
        if (n == 0) { a.grid[at] = -1.0f; ++marked; }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) marked += sf_shfl_xor(marked, o);
  if ((threadIdx.x & 63) == 0) wave_marked[threadIdx.x >> 6] = marked;
  sf_sync();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (int w = 0; w < OCC_MARK_BLOCK / 64; ++w) total += wave_marked[w];
    if (total) occ_mark_add(a.n_marked, total);
  }
}

// The occupancy-grid marcher of raymarch_occ.hip (march_rays_train / march_rays, raymarching/src/raymarching.cu:302-492, :695-818):
// the state of one marching ray and its two steps, `probe` and `skip`.  Written against sf_dev.h / ngp_device.h so that the kernels of
// raymarch_occ.hip and the host emulation of tests/hostemu (ngp_occ_shade.h through occ_shade_emu.cpp) compile the same source.
// fp32 arithmetic is written with the contraction nvcc applies (-fmad=true) as explicit fmaf.  For a grid size H that is a power of two
// (128 everywhere in this project; Morton order presumes it) every other product that feeds a sum here is exact -- a factor 2 or 0.5, or
// `level * H^3`, a small integer times a power of two -- so a build that contracts and one that does not give the same bits.  For any
// other H (the C entries accept 1..1024) `level * H^3` in `probe` can round, and a contracted build may then pick a different cell than
// a non-contracting one: the host emulation and the device are only known to agree for power-of-two H.
#pragma once
#include <float.h>
#include "sf_dev.h"
#include "ngp_device.h"

#define SF_SQRT3 1.7320508075688772f

SF_DEV float clampf(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }
SF_DEV float signf1(float x) { return copysignf(1.0f, x); }

SF_DEV uint32_t occ_expand_bits(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

SF_DEV int mip_from_pos(float x, float y, float z, float max_cascade) {
  const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
  int e;
  (void)frexpf(mx, &e);
  return (int)fminf(max_cascade - 1.0f, fmaxf(0.0f, (float)e));
}
SF_DEV int mip_from_dt(float dt, float H, float max_cascade) {
  const float mx = (float)((double)(dt * H) * 0.5);
  int e;
  (void)frexpf(mx, &e);
  return (int)fminf(max_cascade - 1.0f, fmaxf(0.0f, (float)e));
}

// State of one marching ray; `probe` classifies the sample at the current t, `skip` jumps an empty cell.
struct Marcher {
  float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz, rH, H3, bound, dt_gamma, dt_min, dt_max;
  uint32_t C, H;
  const uint8_t* grid;

  SF_DEV void init(const float* o, const float* d, const uint8_t* g, float bnd, float gamma,
                   uint32_t max_steps, uint32_t c, uint32_t h) {
    ox = o[0]; oy = o[1]; oz = o[2]; dx = d[0]; dy = d[1]; dz = d[2];
    rdx = SF_DIV(1.0f, dx); rdy = SF_DIV(1.0f, dy); rdz = SF_DIV(1.0f, dz);
    rH = SF_DIV(1.0f, (float)h);
    H3 = (float)(h * h * h);
    bound = bnd; dt_gamma = gamma; C = c; H = h; grid = g;
    dt_min = SF_DIV(2.0f * SF_SQRT3, (float)max_steps);
    dt_max = SF_DIV(2.0f * SF_SQRT3 * (float)(1 << (c - 1)), (float)h);
  }
  SF_DEV float step_size(float t) const { return clampf(t * dt_gamma, dt_min, dt_max); }

  // returns occupancy of the cell holding the sample at t; fills the clamped position, dt and the cell geometry
  SF_DEV bool probe(float t, float& x, float& y, float& z, float& dt, int& nx, int& ny, int& nz,
                    float& mip_bound) const {
    x = clampf(fmaf(t, dx, ox), -bound, bound);
    y = clampf(fmaf(t, dy, oy), -bound, bound);
    z = clampf(fmaf(t, dz, oz), -bound, bound);
    dt = step_size(t);
    const int l0 = mip_from_pos(x, y, z, (float)C), l1 = mip_from_dt(dt, (float)H, (float)C);
    const int level = l0 > l1 ? l0 : l1;
    mip_bound = fminf(scalbnf(1.0f, level), bound);
    const float mip_rbound = SF_DIV(1.0f, mip_bound);
    const float hi = (float)(H - 1);
    // `0.5 * (...) * H` is evaluated in double (0.5 is a double literal), then narrowed for clamp()
    nx = (int)clampf((float)(0.5 * (double)fmaf(x, mip_rbound, 1.0f) * (double)H), 0.0f, hi);
    ny = (int)clampf((float)(0.5 * (double)fmaf(y, mip_rbound, 1.0f) * (double)H), 0.0f, hi);
    nz = (int)clampf((float)(0.5 * (double)fmaf(z, mip_rbound, 1.0f) * (double)H), 0.0f, hi);
    // level * H3 is a float product converted to uint32 after the integer Morton code is added in float
    const uint32_t morton = occ_expand_bits((uint32_t)nx) | (occ_expand_bits((uint32_t)ny) << 1) | (occ_expand_bits((uint32_t)nz) << 2);
    const uint32_t index = (uint32_t)((float)level * H3 + (float)morton);
    return (grid[index >> 3] >> (index & 7u)) & 1u;
  }
  // advance t past the empty cell (nx, ny, nz)
  SF_DEV float skip(float t, float x, float y, float z, int nx, int ny, int nz, float mip_bound) const {
    const float tx = (fmaf(((float)nx + 0.5f + 0.5f * signf1(dx)) * rH * 2.0f - 1.0f, mip_bound, -x)) * rdx;
    const float ty = (fmaf(((float)ny + 0.5f + 0.5f * signf1(dy)) * rH * 2.0f - 1.0f, mip_bound, -y)) * rdy;
    const float tz = (fmaf(((float)nz + 0.5f + 0.5f * signf1(dz)) * rH * 2.0f - 1.0f, mip_bound, -z)) * rdz;
    const float tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
    do { t += step_size(t); } while (t < tt);
    return t;
  }
};

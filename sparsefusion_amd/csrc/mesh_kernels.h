// Mesh export kernels (gfx950): separable 3-D Gaussian with fused fp64 volume statistics, and marching cubes in two phases
// (classify + scan -> counts, then emit) with one canonical output order.  Plain C++ over sf_dev.h, so tests/hostemu compiles the
// same source for the CPU; the host entry points and the NGP density lattice are in mesh.hip.  See DESIGN.md section 9.
//
// Layouts: a volume is [nx][ny][nz] float32, point p = (i * ny + j) * nz + k.
//
// Gaussian (mcubes.smooth_gaussian = scipy.ndimage.gaussian_filter, mode 'reflect'): one pass per axis in the order 0, 1, 2, the
// taps normalised on the host in double; each output accumulates in double and is rounded to fp32.  The two strided axes give
// each thread one column segment (consecutive threads take consecutive inner indices: coalesced); the contiguous axis stages a
// row tile in LDS.  The last pass also writes per-workgroup partial sums of x and x^2 (double, fixed order); one workgroup then
// adds the partials in fixed order -- no floating-point atomics, so the mean / std are bit-reproducible.
//
// Marching cubes (Lorensen / Bourke corner and edge numbering and 256 x 16 triangle table; a corner is inside when v < iso):
//   classify  per point: the 3-bit mask of its OWNED crossing edges (toward +x, +y, +z) and, for a cell (i < nx-1, ..), its cube
//             index; per workgroup of MC_BLOCK points: the vertex and triangle counts.
//   scan      one workgroup: exclusive prefix sums of the workgroup counts (any number of workgroups), totals (V, F).
//   emit      vertices: vertex ids in point-major x-major order, then axis x < y < z; the owning point computes its vertex once
//             (a + t, t = (iso - v_a) / (v_b - v_a), fp32, no contraction) and records its first id.  Faces: cell x-major order,
//             then table order; a face corner is vbase[owner] + popcount(mask[owner] & ((1 << axis) - 1)) of the edge's owner.
//   With inside = v < iso the table's winding makes every face look toward decreasing field values (outward on a density blob).
#pragma once
#include "sf_dev.h"

#define GS_NT 256            // threads of every Gaussian workgroup
#define GS_RMAX 64           // largest supported radius (int(truncate * sigma + 0.5))
#define GS_SEG 16            // outputs per thread of a strided pass
#define GS_STAT_WG 2048      // workgroups of the last (contiguous) pass = partial sums the statistics add
#define MC_NT 256
#define MC_ITEMS 4           // consecutive points per thread
#define MC_BLOCK (MC_NT * MC_ITEMS)

struct GaussTaps { double w[2 * GS_RMAX + 1]; int r; };

// host: the taps of scipy.ndimage._gaussian_kernel1d in double -- radius int(truncate * sigma + 0.5), exp(-x^2 / (2 sigma^2))
// normalised.  false when sigma <= 0, truncate < 0 or the radius exceeds GS_RMAX.
static inline bool gs_make_taps(float sigma, float truncate, GaussTaps* t) {
  const double sd = (double)sigma, rr = (double)truncate * sd + 0.5;
  if (!(sigma > 0.0f) || !(truncate >= 0.0f) || !(rr < GS_RMAX + 1)) return false;
  *t = GaussTaps{};
  t->r = (int)rr;
  double sum = 0.0;
  for (int q = -t->r; q <= t->r; ++q) sum += (t->w[q + t->r] = exp(-0.5 / (sd * sd) * (double)q * (double)q));
  for (int q = 0; q <= 2 * t->r; ++q) t->w[q] /= sum;
  return true;
}

// scipy 'reflect' (d c b a | a b c d | d c b a), repeated for any distance: a dimension shorter than the radius reflects again
SF_DEV uint32_t gs_reflect(int64_t m, uint32_t n) {
  const int64_t period = 2 * (int64_t)n;
  int64_t q = m % period;
  if (q < 0) q += period;
  return (uint32_t)(q < (int64_t)n ? q : period - 1 - q);
}

// one strided axis: the volume viewed as [outer][n][inner], filtered along n; thread = (inner index, segment of GS_SEG outputs, outer)
SF_KERNEL(GS_NT) void k_gauss_strided(const float* __restrict__ in, float* __restrict__ out, uint32_t outer, uint32_t n, uint32_t inner,
                                     GaussTaps taps) {
  const uint32_t nseg = (n + GS_SEG - 1) / GS_SEG;
  const uint64_t t = (uint64_t)blockIdx.x * GS_NT + threadIdx.x;
  if (t >= (uint64_t)outer * nseg * inner) return;
  const uint32_t c = (uint32_t)(t % inner);
  const uint64_t rest = t / inner;
  const uint32_t seg = (uint32_t)(rest % nseg), o = (uint32_t)(rest / nseg);
  const uint64_t base = (uint64_t)o * n * inner + c;
  const uint32_t s1 = seg * GS_SEG + GS_SEG < n ? seg * GS_SEG + GS_SEG : n;
  for (uint32_t s = seg * GS_SEG; s < s1; ++s) {
    double acc = 0.0;
    for (int q = -taps.r; q <= taps.r; ++q) acc += taps.w[q + taps.r] * (double)in[base + (uint64_t)gs_reflect((int64_t)s + q, n) * inner];
    out[base + (uint64_t)s * inner] = (float)acc;
  }
}

// the contiguous axis: tiles of GS_NT outputs of one row (row = [nz] floats), staged with their halo in LDS; every workgroup walks
// tiles blockIdx.x, + gridDim.x, .. and, when `partial` is given, writes its sum of x and x^2 (double) to partial[2 * blockIdx.x ..]
SF_KERNEL(GS_NT) void k_gauss_rows(const float* __restrict__ in, float* __restrict__ out, uint64_t rows, uint32_t n, GaussTaps taps,
                                  double* __restrict__ partial) {
  SF_SHARED float tile[GS_NT + 2 * GS_RMAX];
  SF_SHARED double red[2][GS_NT];
  const uint32_t tid = threadIdx.x;
  const uint32_t ntile = (n + GS_NT - 1) / GS_NT;
  const int r = taps.r;
  double s1 = 0.0, s2 = 0.0;
  for (uint64_t tt = blockIdx.x; tt < rows * ntile; tt += gridDim.x) {
    const uint64_t row = tt / ntile;
    const int64_t k0 = (int64_t)(tt % ntile) * GS_NT;
    const float* src = in + row * n;
    for (int q = (int)tid; q < GS_NT + 2 * r; q += GS_NT) tile[q] = src[gs_reflect(k0 - r + q, n)];
    sf_sync();
    if (k0 + tid < n) {
      double acc = 0.0;
      for (int q = 0; q <= 2 * r; ++q) acc += taps.w[q] * (double)tile[tid + q];
      const float v = (float)acc;
      out[row * n + k0 + tid] = v;
      s1 += (double)v;
      s2 += (double)v * (double)v;
    }
    sf_sync();
  }
  if (!partial) return;
  red[0][tid] = s1;
  red[1][tid] = s2;
  sf_sync();
  for (uint32_t o = GS_NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    sf_sync();
  }
  if (tid == 0) {
    partial[2 * blockIdx.x] = red[0][0];
    partial[2 * blockIdx.x + 1] = red[1][0];
  }
}

// one workgroup: stats = {mean, population std} of `count` values from nblk partial pairs, added in a fixed order
SF_KERNEL(GS_NT) void k_gauss_stats(const double* __restrict__ partial, uint32_t nblk, uint64_t count, double* __restrict__ stats) {
  SF_SHARED double red[2][GS_NT];
  const uint32_t tid = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (uint32_t b = tid; b < nblk; b += GS_NT) {
    s1 += partial[2 * b];
    s2 += partial[2 * b + 1];
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  sf_sync();
  for (uint32_t o = GS_NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    sf_sync();
  }
  if (tid == 0) {
    const double mean = red[0][0] / (double)count;
    const double var = red[1][0] / (double)count - mean * mean;
    stats[0] = mean;
    stats[1] = sqrt(var > 0.0 ? var : 0.0);
  }
}

// ------------------------------------------------------------------------------------------------------------- marching cubes
// edge e -> owner point offset (dx, dy, dz) and axis (the lower corner of the edge owns it)
SF_CONSTANT int8_t mc_edge_owner[12][4] = {
    {0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}, {1, 0, 1, 1},
    {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};
// corner c of the classic numbering at (dx, dy, dz)
SF_CONSTANT int8_t mc_corner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
// triangles of each cube configuration (bit c of the index set = corner c inside), -1 terminated
SF_CONSTANT int8_t mc_tri[256][16] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 8, 3, 9, 8, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 8, 3, 1, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {9, 2, 10, 0, 2, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 8, 3, 2, 10, 8, 10, 9, 8, -1, -1, -1, -1, -1, -1, -1}, {3, 11, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 2, 8, 11, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 9, 0, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 11, 2, 1, 9, 11, 9, 8, 11, -1, -1, -1, -1, -1, -1, -1}, {3, 10, 1, 11, 10, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 10, 1, 0, 8, 10, 8, 11, 10, -1, -1, -1, -1, -1, -1, -1}, {3, 9, 0, 3, 11, 9, 11, 10, 9, -1, -1, -1, -1, -1, -1, -1},
    {9, 8, 10, 10, 8, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 3, 0, 7, 3, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 8, 4, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 1, 9, 4, 7, 1, 7, 3, 1, -1, -1, -1, -1, -1, -1, -1}, {1, 2, 10, 8, 4, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 4, 7, 3, 0, 4, 1, 2, 10, -1, -1, -1, -1, -1, -1, -1}, {9, 2, 10, 9, 0, 2, 8, 4, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 10, 9, 2, 9, 7, 2, 7, 3, 7, 9, 4, -1, -1, -1, -1}, {8, 4, 7, 3, 11, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {11, 4, 7, 11, 2, 4, 2, 0, 4, -1, -1, -1, -1, -1, -1, -1}, {9, 0, 1, 8, 4, 7, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1},
    {4, 7, 11, 9, 4, 11, 9, 11, 2, 9, 2, 1, -1, -1, -1, -1}, {3, 10, 1, 3, 11, 10, 7, 8, 4, -1, -1, -1, -1, -1, -1, -1},
    {1, 11, 10, 1, 4, 11, 1, 0, 4, 7, 11, 4, -1, -1, -1, -1}, {4, 7, 8, 9, 0, 11, 9, 11, 10, 11, 0, 3, -1, -1, -1, -1},
    {4, 7, 11, 4, 11, 9, 9, 11, 10, -1, -1, -1, -1, -1, -1, -1}, {9, 5, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {9, 5, 4, 0, 8, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 5, 4, 1, 5, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {8, 5, 4, 8, 3, 5, 3, 1, 5, -1, -1, -1, -1, -1, -1, -1}, {1, 2, 10, 9, 5, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {3, 0, 8, 1, 2, 10, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1}, {5, 2, 10, 5, 4, 2, 4, 0, 2, -1, -1, -1, -1, -1, -1, -1},
    {2, 10, 5, 3, 2, 5, 3, 5, 4, 3, 4, 8, -1, -1, -1, -1}, {9, 5, 4, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 11, 2, 0, 8, 11, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1}, {0, 5, 4, 0, 1, 5, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1},
    {2, 1, 5, 2, 5, 8, 2, 8, 11, 4, 8, 5, -1, -1, -1, -1}, {10, 3, 11, 10, 1, 3, 9, 5, 4, -1, -1, -1, -1, -1, -1, -1},
    {4, 9, 5, 0, 8, 1, 8, 10, 1, 8, 11, 10, -1, -1, -1, -1}, {5, 4, 0, 5, 0, 11, 5, 11, 10, 11, 0, 3, -1, -1, -1, -1},
    {5, 4, 8, 5, 8, 10, 10, 8, 11, -1, -1, -1, -1, -1, -1, -1}, {9, 7, 8, 5, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {9, 3, 0, 9, 5, 3, 5, 7, 3, -1, -1, -1, -1, -1, -1, -1}, {0, 7, 8, 0, 1, 7, 1, 5, 7, -1, -1, -1, -1, -1, -1, -1},
    {1, 5, 3, 3, 5, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {9, 7, 8, 9, 5, 7, 10, 1, 2, -1, -1, -1, -1, -1, -1, -1},
    {10, 1, 2, 9, 5, 0, 5, 3, 0, 5, 7, 3, -1, -1, -1, -1}, {8, 0, 2, 8, 2, 5, 8, 5, 7, 10, 5, 2, -1, -1, -1, -1},
    {2, 10, 5, 2, 5, 3, 3, 5, 7, -1, -1, -1, -1, -1, -1, -1}, {7, 9, 5, 7, 8, 9, 3, 11, 2, -1, -1, -1, -1, -1, -1, -1},
    {9, 5, 7, 9, 7, 2, 9, 2, 0, 2, 7, 11, -1, -1, -1, -1}, {2, 3, 11, 0, 1, 8, 1, 7, 8, 1, 5, 7, -1, -1, -1, -1},
    {11, 2, 1, 11, 1, 7, 7, 1, 5, -1, -1, -1, -1, -1, -1, -1}, {9, 5, 8, 8, 5, 7, 10, 1, 3, 10, 3, 11, -1, -1, -1, -1},
    {5, 7, 0, 5, 0, 9, 7, 11, 0, 1, 0, 10, 11, 10, 0, -1}, {11, 10, 0, 11, 0, 3, 10, 5, 0, 8, 0, 7, 5, 7, 0, -1},
    {11, 10, 5, 7, 11, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {10, 6, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {9, 0, 1, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 8, 3, 1, 9, 8, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1},
    {1, 6, 5, 2, 6, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 6, 5, 1, 2, 6, 3, 0, 8, -1, -1, -1, -1, -1, -1, -1},
    {9, 6, 5, 9, 0, 6, 0, 2, 6, -1, -1, -1, -1, -1, -1, -1}, {5, 9, 8, 5, 8, 2, 5, 2, 6, 3, 2, 8, -1, -1, -1, -1},
    {2, 3, 11, 10, 6, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {11, 0, 8, 11, 2, 0, 10, 6, 5, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 9, 2, 3, 11, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1}, {5, 10, 6, 1, 9, 2, 9, 11, 2, 9, 8, 11, -1, -1, -1, -1},
    {6, 3, 11, 6, 5, 3, 5, 1, 3, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 11, 0, 11, 5, 0, 5, 1, 5, 11, 6, -1, -1, -1, -1},
    {3, 11, 6, 0, 3, 6, 0, 6, 5, 0, 5, 9, -1, -1, -1, -1}, {6, 5, 9, 6, 9, 11, 11, 9, 8, -1, -1, -1, -1, -1, -1, -1},
    {5, 10, 6, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {4, 3, 0, 4, 7, 3, 6, 5, 10, -1, -1, -1, -1, -1, -1, -1},
    {1, 9, 0, 5, 10, 6, 8, 4, 7, -1, -1, -1, -1, -1, -1, -1}, {10, 6, 5, 1, 9, 7, 1, 7, 3, 7, 9, 4, -1, -1, -1, -1},
    {6, 1, 2, 6, 5, 1, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1}, {1, 2, 5, 5, 2, 6, 3, 0, 4, 3, 4, 7, -1, -1, -1, -1},
    {8, 4, 7, 9, 0, 5, 0, 6, 5, 0, 2, 6, -1, -1, -1, -1}, {7, 3, 9, 7, 9, 4, 3, 2, 9, 5, 9, 6, 2, 6, 9, -1},
    {3, 11, 2, 7, 8, 4, 10, 6, 5, -1, -1, -1, -1, -1, -1, -1}, {5, 10, 6, 4, 7, 2, 4, 2, 0, 2, 7, 11, -1, -1, -1, -1},
    {0, 1, 9, 4, 7, 8, 2, 3, 11, 5, 10, 6, -1, -1, -1, -1}, {9, 2, 1, 9, 11, 2, 9, 4, 11, 7, 11, 4, 5, 10, 6, -1},
    {8, 4, 7, 3, 11, 5, 3, 5, 1, 5, 11, 6, -1, -1, -1, -1}, {5, 1, 11, 5, 11, 6, 1, 0, 11, 7, 11, 4, 0, 4, 11, -1},
    {0, 5, 9, 0, 6, 5, 0, 3, 6, 11, 6, 3, 8, 4, 7, -1}, {6, 5, 9, 6, 9, 11, 4, 7, 9, 7, 11, 9, -1, -1, -1, -1},
    {10, 4, 9, 6, 4, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {4, 10, 6, 4, 9, 10, 0, 8, 3, -1, -1, -1, -1, -1, -1, -1},
    {10, 0, 1, 10, 6, 0, 6, 4, 0, -1, -1, -1, -1, -1, -1, -1}, {8, 3, 1, 8, 1, 6, 8, 6, 4, 6, 1, 10, -1, -1, -1, -1},
    {1, 4, 9, 1, 2, 4, 2, 6, 4, -1, -1, -1, -1, -1, -1, -1}, {3, 0, 8, 1, 2, 9, 2, 4, 9, 2, 6, 4, -1, -1, -1, -1},
    {0, 2, 4, 4, 2, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {8, 3, 2, 8, 2, 4, 4, 2, 6, -1, -1, -1, -1, -1, -1, -1},
    {10, 4, 9, 10, 6, 4, 11, 2, 3, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 2, 2, 8, 11, 4, 9, 10, 4, 10, 6, -1, -1, -1, -1},
    {3, 11, 2, 0, 1, 6, 0, 6, 4, 6, 1, 10, -1, -1, -1, -1}, {6, 4, 1, 6, 1, 10, 4, 8, 1, 2, 1, 11, 8, 11, 1, -1},
    {9, 6, 4, 9, 3, 6, 9, 1, 3, 11, 6, 3, -1, -1, -1, -1}, {8, 11, 1, 8, 1, 0, 11, 6, 1, 9, 1, 4, 6, 4, 1, -1},
    {3, 11, 6, 3, 6, 0, 0, 6, 4, -1, -1, -1, -1, -1, -1, -1}, {6, 4, 8, 11, 6, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {7, 10, 6, 7, 8, 10, 8, 9, 10, -1, -1, -1, -1, -1, -1, -1}, {0, 7, 3, 0, 10, 7, 0, 9, 10, 6, 7, 10, -1, -1, -1, -1},
    {10, 6, 7, 1, 10, 7, 1, 7, 8, 1, 8, 0, -1, -1, -1, -1}, {10, 6, 7, 10, 7, 1, 1, 7, 3, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 6, 1, 6, 8, 1, 8, 9, 8, 6, 7, -1, -1, -1, -1}, {2, 6, 9, 2, 9, 1, 6, 7, 9, 0, 9, 3, 7, 3, 9, -1},
    {7, 8, 0, 7, 0, 6, 6, 0, 2, -1, -1, -1, -1, -1, -1, -1}, {7, 3, 2, 6, 7, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 11, 10, 6, 8, 10, 8, 9, 8, 6, 7, -1, -1, -1, -1}, {2, 0, 7, 2, 7, 11, 0, 9, 7, 6, 7, 10, 9, 10, 7, -1},
    {1, 8, 0, 1, 7, 8, 1, 10, 7, 6, 7, 10, 2, 3, 11, -1}, {11, 2, 1, 11, 1, 7, 10, 6, 1, 6, 7, 1, -1, -1, -1, -1},
    {8, 9, 6, 8, 6, 7, 9, 1, 6, 11, 6, 3, 1, 3, 6, -1}, {0, 9, 1, 11, 6, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {7, 8, 0, 7, 0, 6, 3, 11, 0, 11, 6, 0, -1, -1, -1, -1}, {7, 11, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {7, 6, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {3, 0, 8, 11, 7, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 9, 11, 7, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {8, 1, 9, 8, 3, 1, 11, 7, 6, -1, -1, -1, -1, -1, -1, -1},
    {10, 1, 2, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 2, 10, 3, 0, 8, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1},
    {2, 9, 0, 2, 10, 9, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1}, {6, 11, 7, 2, 10, 3, 10, 8, 3, 10, 9, 8, -1, -1, -1, -1},
    {7, 2, 3, 6, 2, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {7, 0, 8, 7, 6, 0, 6, 2, 0, -1, -1, -1, -1, -1, -1, -1},
    {2, 7, 6, 2, 3, 7, 0, 1, 9, -1, -1, -1, -1, -1, -1, -1}, {1, 6, 2, 1, 8, 6, 1, 9, 8, 8, 7, 6, -1, -1, -1, -1},
    {10, 7, 6, 10, 1, 7, 1, 3, 7, -1, -1, -1, -1, -1, -1, -1}, {10, 7, 6, 1, 7, 10, 1, 8, 7, 1, 0, 8, -1, -1, -1, -1},
    {0, 3, 7, 0, 7, 10, 0, 10, 9, 6, 10, 7, -1, -1, -1, -1}, {7, 6, 10, 7, 10, 8, 8, 10, 9, -1, -1, -1, -1, -1, -1, -1},
    {6, 8, 4, 11, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {3, 6, 11, 3, 0, 6, 0, 4, 6, -1, -1, -1, -1, -1, -1, -1},
    {8, 6, 11, 8, 4, 6, 9, 0, 1, -1, -1, -1, -1, -1, -1, -1}, {9, 4, 6, 9, 6, 3, 9, 3, 1, 11, 3, 6, -1, -1, -1, -1},
    {6, 8, 4, 6, 11, 8, 2, 10, 1, -1, -1, -1, -1, -1, -1, -1}, {1, 2, 10, 3, 0, 11, 0, 6, 11, 0, 4, 6, -1, -1, -1, -1},
    {4, 11, 8, 4, 6, 11, 0, 2, 9, 2, 10, 9, -1, -1, -1, -1}, {10, 9, 3, 10, 3, 2, 9, 4, 3, 11, 3, 6, 4, 6, 3, -1},
    {8, 2, 3, 8, 4, 2, 4, 6, 2, -1, -1, -1, -1, -1, -1, -1}, {0, 4, 2, 4, 6, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 9, 0, 2, 3, 4, 2, 4, 6, 4, 3, 8, -1, -1, -1, -1}, {1, 9, 4, 1, 4, 2, 2, 4, 6, -1, -1, -1, -1, -1, -1, -1},
    {8, 1, 3, 8, 6, 1, 8, 4, 6, 6, 10, 1, -1, -1, -1, -1}, {10, 1, 0, 10, 0, 6, 6, 0, 4, -1, -1, -1, -1, -1, -1, -1},
    {4, 6, 3, 4, 3, 8, 6, 10, 3, 0, 3, 9, 10, 9, 3, -1}, {10, 9, 4, 6, 10, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 9, 5, 7, 6, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 4, 9, 5, 11, 7, 6, -1, -1, -1, -1, -1, -1, -1},
    {5, 0, 1, 5, 4, 0, 7, 6, 11, -1, -1, -1, -1, -1, -1, -1}, {11, 7, 6, 8, 3, 4, 3, 5, 4, 3, 1, 5, -1, -1, -1, -1},
    {9, 5, 4, 10, 1, 2, 7, 6, 11, -1, -1, -1, -1, -1, -1, -1}, {6, 11, 7, 1, 2, 10, 0, 8, 3, 4, 9, 5, -1, -1, -1, -1},
    {7, 6, 11, 5, 4, 10, 4, 2, 10, 4, 0, 2, -1, -1, -1, -1}, {3, 4, 8, 3, 5, 4, 3, 2, 5, 10, 5, 2, 11, 7, 6, -1},
    {7, 2, 3, 7, 6, 2, 5, 4, 9, -1, -1, -1, -1, -1, -1, -1}, {9, 5, 4, 0, 8, 6, 0, 6, 2, 6, 8, 7, -1, -1, -1, -1},
    {3, 6, 2, 3, 7, 6, 1, 5, 0, 5, 4, 0, -1, -1, -1, -1}, {6, 2, 8, 6, 8, 7, 2, 1, 8, 4, 8, 5, 1, 5, 8, -1},
    {9, 5, 4, 10, 1, 6, 1, 7, 6, 1, 3, 7, -1, -1, -1, -1}, {1, 6, 10, 1, 7, 6, 1, 0, 7, 8, 7, 0, 9, 5, 4, -1},
    {4, 0, 10, 4, 10, 5, 0, 3, 10, 6, 10, 7, 3, 7, 10, -1}, {7, 6, 10, 7, 10, 8, 5, 4, 10, 4, 8, 10, -1, -1, -1, -1},
    {6, 9, 5, 6, 11, 9, 11, 8, 9, -1, -1, -1, -1, -1, -1, -1}, {3, 6, 11, 0, 6, 3, 0, 5, 6, 0, 9, 5, -1, -1, -1, -1},
    {0, 11, 8, 0, 5, 11, 0, 1, 5, 5, 6, 11, -1, -1, -1, -1}, {6, 11, 3, 6, 3, 5, 5, 3, 1, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 10, 9, 5, 11, 9, 11, 8, 11, 5, 6, -1, -1, -1, -1}, {0, 11, 3, 0, 6, 11, 0, 9, 6, 5, 6, 9, 1, 2, 10, -1},
    {11, 8, 5, 11, 5, 6, 8, 0, 5, 10, 5, 2, 0, 2, 5, -1}, {6, 11, 3, 6, 3, 5, 2, 10, 3, 10, 5, 3, -1, -1, -1, -1},
    {5, 8, 9, 5, 2, 8, 5, 6, 2, 3, 8, 2, -1, -1, -1, -1}, {9, 5, 6, 9, 6, 0, 0, 6, 2, -1, -1, -1, -1, -1, -1, -1},
    {1, 5, 8, 1, 8, 0, 5, 6, 8, 3, 8, 2, 6, 2, 8, -1}, {1, 5, 6, 2, 1, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 6, 1, 6, 10, 3, 8, 6, 5, 6, 9, 8, 9, 6, -1}, {10, 1, 0, 10, 0, 6, 9, 5, 0, 5, 6, 0, -1, -1, -1, -1},
    {0, 3, 8, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {10, 5, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {11, 5, 10, 7, 5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {11, 5, 10, 11, 7, 5, 8, 3, 0, -1, -1, -1, -1, -1, -1, -1},
    {5, 11, 7, 5, 10, 11, 1, 9, 0, -1, -1, -1, -1, -1, -1, -1}, {10, 7, 5, 10, 11, 7, 9, 8, 1, 8, 3, 1, -1, -1, -1, -1},
    {11, 1, 2, 11, 7, 1, 7, 5, 1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 1, 2, 7, 1, 7, 5, 7, 2, 11, -1, -1, -1, -1},
    {9, 7, 5, 9, 2, 7, 9, 0, 2, 2, 11, 7, -1, -1, -1, -1}, {7, 5, 2, 7, 2, 11, 5, 9, 2, 3, 2, 8, 9, 8, 2, -1},
    {2, 5, 10, 2, 3, 5, 3, 7, 5, -1, -1, -1, -1, -1, -1, -1}, {8, 2, 0, 8, 5, 2, 8, 7, 5, 10, 2, 5, -1, -1, -1, -1},
    {9, 0, 1, 5, 10, 3, 5, 3, 7, 3, 10, 2, -1, -1, -1, -1}, {9, 8, 2, 9, 2, 1, 8, 7, 2, 10, 2, 5, 7, 5, 2, -1},
    {1, 3, 5, 3, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 7, 0, 7, 1, 1, 7, 5, -1, -1, -1, -1, -1, -1, -1},
    {9, 0, 3, 9, 3, 5, 5, 3, 7, -1, -1, -1, -1, -1, -1, -1}, {9, 8, 7, 5, 9, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 8, 4, 5, 10, 8, 10, 11, 8, -1, -1, -1, -1, -1, -1, -1}, {5, 0, 4, 5, 11, 0, 5, 10, 11, 11, 3, 0, -1, -1, -1, -1},
    {0, 1, 9, 8, 4, 10, 8, 10, 11, 10, 4, 5, -1, -1, -1, -1}, {10, 11, 4, 10, 4, 5, 11, 3, 4, 9, 4, 1, 3, 1, 4, -1},
    {2, 5, 1, 2, 8, 5, 2, 11, 8, 4, 5, 8, -1, -1, -1, -1}, {0, 4, 11, 0, 11, 3, 4, 5, 11, 2, 11, 1, 5, 1, 11, -1},
    {0, 2, 5, 0, 5, 9, 2, 11, 5, 4, 5, 8, 11, 8, 5, -1}, {9, 4, 5, 2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 5, 10, 3, 5, 2, 3, 4, 5, 3, 8, 4, -1, -1, -1, -1}, {5, 10, 2, 5, 2, 4, 4, 2, 0, -1, -1, -1, -1, -1, -1, -1},
    {3, 10, 2, 3, 5, 10, 3, 8, 5, 4, 5, 8, 0, 1, 9, -1}, {5, 10, 2, 5, 2, 4, 1, 9, 2, 9, 4, 2, -1, -1, -1, -1},
    {8, 4, 5, 8, 5, 3, 3, 5, 1, -1, -1, -1, -1, -1, -1, -1}, {0, 4, 5, 1, 0, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {8, 4, 5, 8, 5, 3, 9, 0, 5, 0, 3, 5, -1, -1, -1, -1}, {9, 4, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 11, 7, 4, 9, 11, 9, 10, 11, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 4, 9, 7, 9, 11, 7, 9, 10, 11, -1, -1, -1, -1},
    {1, 10, 11, 1, 11, 4, 1, 4, 0, 7, 4, 11, -1, -1, -1, -1}, {3, 1, 4, 3, 4, 8, 1, 10, 4, 7, 4, 11, 10, 11, 4, -1},
    {4, 11, 7, 9, 11, 4, 9, 2, 11, 9, 1, 2, -1, -1, -1, -1}, {9, 7, 4, 9, 11, 7, 9, 1, 11, 2, 11, 1, 0, 8, 3, -1},
    {11, 7, 4, 11, 4, 2, 2, 4, 0, -1, -1, -1, -1, -1, -1, -1}, {11, 7, 4, 11, 4, 2, 8, 3, 4, 3, 2, 4, -1, -1, -1, -1},
    {2, 9, 10, 2, 7, 9, 2, 3, 7, 7, 4, 9, -1, -1, -1, -1}, {9, 10, 7, 9, 7, 4, 10, 2, 7, 8, 7, 0, 2, 0, 7, -1},
    {3, 7, 10, 3, 10, 2, 7, 4, 10, 1, 10, 0, 4, 0, 10, -1}, {1, 10, 2, 8, 7, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 9, 1, 4, 1, 7, 7, 1, 3, -1, -1, -1, -1, -1, -1, -1}, {4, 9, 1, 4, 1, 7, 0, 8, 1, 8, 7, 1, -1, -1, -1, -1},
    {4, 0, 3, 7, 4, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {9, 10, 8, 10, 11, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {3, 0, 9, 3, 9, 11, 11, 9, 10, -1, -1, -1, -1, -1, -1, -1},
    {0, 1, 10, 0, 10, 8, 8, 10, 11, -1, -1, -1, -1, -1, -1, -1}, {3, 1, 10, 11, 3, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 11, 1, 11, 9, 9, 11, 8, -1, -1, -1, -1, -1, -1, -1}, {3, 0, 9, 3, 9, 11, 1, 2, 9, 2, 11, 9, -1, -1, -1, -1},
    {0, 2, 11, 8, 0, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {3, 2, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 8, 2, 8, 10, 10, 8, 9, -1, -1, -1, -1, -1, -1, -1}, {9, 10, 2, 0, 9, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 8, 2, 8, 10, 0, 1, 8, 1, 10, 8, -1, -1, -1, -1}, {1, 10, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 8, 9, 1, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 9, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {0, 3, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}
};

struct McDims { uint32_t nx, ny, nz; };

// position of a vertex along its edge: a + (iso - v_a) / (v_b - v_a), fp32, one rounding per operation (the division is IEEE:
// hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt)
SF_DEV float mc_vertex(float a, float iso, float va, float vb) {
#pragma clang fp contract(off)
  return a + (iso - va) / (vb - va);
}

SF_DEV uint32_t mc_ntri(uint32_t cube) {
  uint32_t n = 0;
  while (n < 5 && mc_tri[cube][3 * n] >= 0) ++n;
  return n;
}

// code of point p: bits 0-2 owned crossing edges (x, y, z), bits 8-15 cube index of the cell whose lower corner p is (0 if none)
SF_DEV uint32_t mc_code(const float* __restrict__ vol, McDims d, float iso, uint64_t p) {
  const uint32_t k = (uint32_t)(p % d.nz), j = (uint32_t)((p / d.nz) % d.ny), i = (uint32_t)(p / ((uint64_t)d.nz * d.ny));
  const uint64_t sx = (uint64_t)d.ny * d.nz, sy = d.nz;
  const bool in0 = vol[p] < iso;
  uint32_t mask = 0;
  if (i + 1 < d.nx && ((vol[p + sx] < iso) != in0)) mask |= 1u;
  if (j + 1 < d.ny && ((vol[p + sy] < iso) != in0)) mask |= 2u;
  if (k + 1 < d.nz && ((vol[p + 1] < iso) != in0)) mask |= 4u;
  uint32_t cube = 0;
  if (i + 1 < d.nx && j + 1 < d.ny && k + 1 < d.nz) {
    for (int c = 0; c < 8; ++c)
      if (vol[p + mc_corner[c][0] * sx + mc_corner[c][1] * sy + mc_corner[c][2]] < iso) cube |= 1u << c;
  }
  return mask | cube << 8;
}

// exclusive scan of one value per thread over the workgroup (MC_NT threads); returns the thread's offset, *total the sum
SF_DEV uint32_t mc_block_scan(uint32_t v, uint32_t* total) {
  SF_SHARED uint32_t buf[2][MC_NT];
  const uint32_t tid = threadIdx.x;
  int cur = 0;
  buf[0][tid] = v;
  sf_sync();
  for (uint32_t o = 1; o < MC_NT; o <<= 1) {
    const uint32_t x = buf[cur][tid] + (tid >= o ? buf[cur][tid - o] : 0u);
    buf[cur ^ 1][tid] = x;
    cur ^= 1;
    sf_sync();
  }
  const uint32_t incl = buf[cur][tid];
  *total = buf[cur][MC_NT - 1];
  sf_sync();                                        // the buffer is reused by the next call
  return incl - v;
}

// phase 1: codes of every point; per workgroup the number of vertices and triangles of its MC_BLOCK points -> bsum[2 * b ..]
SF_KERNEL(MC_NT) void k_mc_classify(const float* __restrict__ vol, McDims d, float iso, uint16_t* __restrict__ code,
                                   uint32_t* __restrict__ bsum) {
  const uint64_t N = (uint64_t)d.nx * d.ny * d.nz;
  const uint64_t p0 = (uint64_t)blockIdx.x * MC_BLOCK + (uint64_t)threadIdx.x * MC_ITEMS;
  uint32_t nv = 0, nf = 0;
  for (uint32_t u = 0; u < MC_ITEMS; ++u) {
    const uint64_t p = p0 + u;
    if (p >= N) break;
    const uint32_t c = mc_code(vol, d, iso, p);
    code[p] = (uint16_t)c;
    nv += (uint32_t)__builtin_popcount(c & 7u);
    nf += mc_ntri(c >> 8);
  }
  uint32_t tv, tf;
  mc_block_scan(nv, &tv);
  mc_block_scan(nf, &tf);
  if (threadIdx.x == 0) {
    bsum[2 * blockIdx.x] = tv;
    bsum[2 * blockIdx.x + 1] = tf;
  }
}

// phase 1b, one workgroup: boff = exclusive prefix sums of bsum (vertex and triangle counts), counts = {V, F}
SF_KERNEL(MC_NT) void k_mc_scan(const uint32_t* __restrict__ bsum, uint32_t nblk, uint32_t* __restrict__ boff, uint32_t* __restrict__ counts) {
  uint32_t carry_v = 0, carry_f = 0;
  for (uint32_t b0 = 0; b0 < nblk; b0 += MC_NT) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t v = b < nblk ? bsum[2 * b] : 0u, f = b < nblk ? bsum[2 * b + 1] : 0u;
    uint32_t tv, tf;
    const uint32_t ov = mc_block_scan(v, &tv), of = mc_block_scan(f, &tf);
    if (b < nblk) {
      boff[2 * b] = carry_v + ov;
      boff[2 * b + 1] = carry_f + of;
    }
    carry_v += tv;
    carry_f += tf;
  }
  if (threadIdx.x == 0) {
    counts[0] = carry_v;
    counts[1] = carry_f;
  }
}

// phase 2a: vertices, and vbase[p] = id of point p's first vertex
SF_KERNEL(MC_NT) void k_mc_emit_verts(const float* __restrict__ vol, McDims d, float iso, const uint16_t* __restrict__ code,
                                     const uint32_t* __restrict__ boff, float* __restrict__ verts, uint32_t* __restrict__ vbase) {
  const uint64_t N = (uint64_t)d.nx * d.ny * d.nz;
  const uint64_t p0 = (uint64_t)blockIdx.x * MC_BLOCK + (uint64_t)threadIdx.x * MC_ITEMS;
  uint32_t m[MC_ITEMS], nv = 0;
  for (uint32_t u = 0; u < MC_ITEMS; ++u) {
    m[u] = p0 + u < N ? code[p0 + u] & 7u : 0u;
    nv += (uint32_t)__builtin_popcount(m[u]);
  }
  uint32_t tot;
  uint32_t id = boff[2 * blockIdx.x] + mc_block_scan(nv, &tot);
  const uint64_t st[3] = {(uint64_t)d.ny * d.nz, d.nz, 1};
  for (uint32_t u = 0; u < MC_ITEMS; ++u) {
    const uint64_t p = p0 + u;
    if (p >= N) break;
    vbase[p] = id;
    if (!m[u]) continue;
    const uint32_t k = (uint32_t)(p % d.nz), j = (uint32_t)((p / d.nz) % d.ny), i = (uint32_t)(p / st[0]);
    const float va = vol[p];
    for (int a = 0; a < 3; ++a) {
      if (!(m[u] >> a & 1u)) continue;
      float x[3] = {(float)i, (float)j, (float)k};
      x[a] = mc_vertex(x[a], iso, va, vol[p + st[a]]);
      verts[3 * (uint64_t)id + 0] = x[0];
      verts[3 * (uint64_t)id + 1] = x[1];
      verts[3 * (uint64_t)id + 2] = x[2];
      ++id;
    }
  }
}

// phase 2b: faces [F][3] int32 in cell x-major order, then table order
SF_KERNEL(MC_NT) void k_mc_emit_faces(McDims d, const uint16_t* __restrict__ code, const uint32_t* __restrict__ boff,
                                     const uint32_t* __restrict__ vbase, int32_t* __restrict__ faces) {
  const uint64_t N = (uint64_t)d.nx * d.ny * d.nz;
  const uint64_t p0 = (uint64_t)blockIdx.x * MC_BLOCK + (uint64_t)threadIdx.x * MC_ITEMS;
  uint32_t cube[MC_ITEMS], nf = 0;
  for (uint32_t u = 0; u < MC_ITEMS; ++u) {
    cube[u] = p0 + u < N ? code[p0 + u] >> 8 : 0u;
    nf += mc_ntri(cube[u]);
  }
  uint32_t tot;
  uint32_t f = boff[2 * blockIdx.x + 1] + mc_block_scan(nf, &tot);
  const uint64_t sx = (uint64_t)d.ny * d.nz, sy = d.nz;
  for (uint32_t u = 0; u < MC_ITEMS; ++u) {
    const uint32_t c = cube[u];
    for (uint32_t s = 0; s < 5 && mc_tri[c][3 * s] >= 0; ++s, ++f) {
      for (int q = 0; q < 3; ++q) {
        const int e = mc_tri[c][3 * s + q];
        const uint64_t o = p0 + u + mc_edge_owner[e][0] * sx + mc_edge_owner[e][1] * sy + mc_edge_owner[e][2];
        const uint32_t a = (uint32_t)mc_edge_owner[e][3];
        faces[3 * (uint64_t)f + q] = (int32_t)(vbase[o] + (uint32_t)__builtin_popcount(code[o] & 7u & ((1u << a) - 1u)));
      }
    }
  }
}

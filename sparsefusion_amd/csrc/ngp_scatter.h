// Table-gradient scatter of the fused Instant-NGP render backward with device atomics: k_ngp_scatter (the levels whose cell is larger
// than the footprint of a ray patch, summed in an LDS cache first) and k_ngp_scatter_fine (per-corner atomics, for tables too large for
// the binned scatter of ngp_scatter_bin.h).  Written against sf_dev.h like every other backward kernel, so tests/hostemu runs the same
// source on CPU fibres (tests/hostemu/ngp_scatter_emu.cpp); launched by ngp_bwd_field_scatter (ngp_render.hip) as ngp_bwd_plan.h plans.
// k_ngp_scatter_fine takes one by-value SCArgs and the shared helpers (ngp_sample_x01, ngp_z_dropped, sc_corner).  k_ngp_scatter, which
// is on the path of every teacher-field backward, keeps its positional __restrict__ arguments and its own text for the sample point and
// the z-dropped rule: with them hipcc emits the code it always did, line for line, and every other form tried changed it (see there).
//
// Device-memory fp32 atomics execute at the memory side on MI355X (the 8 XCD L2s are not coherent): ~17 G scattered lane-ops/s, so the
// scatter is bound by the NUMBER of atomics.  One workgroup owns a tile of 64 rays (an 8x8 image patch when the ray layout is known) =
// 8192 sorted samples, and walks the levels one at a time:
//   * coarse levels (cell larger than the patch footprint): contributions are first summed in an LDS direct-mapped cache keyed by table
//     row (LDS atomics are ~free), then each touched row is flushed with ONE pair of global atomics per workgroup -- >95 % fewer global
//     atomics on levels 0-5;
//   * fine levels: direct global atomics, z-corner pairs merged on z-dropped levels (ngp_scatter rule, ngp_device.h).
// Reference semantics: external/gridencoder/src/gridencoder.cu:203-262 (kernel_grid_backward: atomicAdd per corner and channel).
#pragma once
#include "sf_dev.h"
#include "ngp_device.h"
#include "ngp_point_attrs.h"                       // ngp_sample_x01 (k_ngp_scatter_fine), ngp_offset_point (k_ngp_scatter's own text)

#define SC_RAYS 64
#define SC_SLOTS 4096
#define SC_EMPTY 0xffffffffu                       // the tag of a free slot: no table row has this index (a level holds < 2^32 rows)
#ifndef SC_RUN
#define SC_RUN 32u              // sorted samples merged per thread before the cache (`sc_run` below; measured with the level split, ngp_bwd_plan.h)
#endif
#define SC_LDS_BYTES ((size_t)SC_SLOTS * (sizeof(uint32_t) + 2 * sizeof(long long)))

// The arguments of k_ngp_scatter_fine.
struct SCArgs {
  NgpLevels lv;
  float bound;
  const float* rays_o; const float* rays_d; const float* aabb; const float* z_s;   // pre-offset to this launch's first ray
  const float* dfeat;          // level-major [L][P_stride][2]
  long long* gtable;           // fixed-point table-gradient sums (sf_dev.h)
  float* gtable_f;             // the fp32 table gradient (addends >= thr, sf_grad_add)
  float thr;
  uint32_t N, T2;              // rays of this launch, sorted samples per ray
  // levels [first_level, L); the launch walks the N rays behind the (pre-offset) ray / sample pointers = points
  // [p_off, p_off + N * T2) of a set of P_stride points, whose level-major layout dfeat keeps
  uint32_t first_level, P_stride, p_off;
  uint32_t off_e; float off_eps;             // OFF = 1 only: offset point off_e = 1 .. 6 of every sample, step off_eps (ngp_point_attrs.h)
};

// x-corner `xb` of the (y, z) corner pair yz = 0 .. 3 of a cell: its table row and weight.  On a z-dropped level corners i and i + 4 share
// their row, so the pairs yz >= 2 are skipped by the caller and the two z-weights are folded here.
SF_DEV void sc_corner(const NgpCell& c, bool z_dropped, int yz, uint32_t xb, uint32_t& row, float& w) {
  const int i0 = yz << 1, i1 = i0 | 1;        // the two x-corners of this (y, z) corner pair
  const float w0 = z_dropped ? SF_ADD(c.w[i0 & 3], c.w[(i0 & 3) + 4]) : c.w[i0];
  const float w1 = z_dropped ? SF_ADD(c.w[i1 & 3], c.w[(i1 & 3) + 4]) : c.w[i1];
  w = xb ? w1 : w0;
  row = xb ? c.row[i1] : c.row[i0];
}

// NT threads share one 80 KB LDS cache (4096 slots of 64-bit fixed-point sums; r02: 8192 of floats) (one workgroup per CU): NT = 1024 puts 4 waves on every SIMD -- the loop body is a
// chain of dependent global loads, hash arithmetic and LDS atomics, and with the first version's 256 threads (ONE wave per
// SIMD) every one of those latencies was exposed.
// Levels [0, last_level) are walked, [0, cached_levels) of them through the LDS cache; rays_per_row = 0: no image layout.
// OFF = 1 (here and in k_ngp_scatter_fine): the points are offset point off_e (1 .. 6, ngp_point_attrs.h) of every sample, step
// off_eps -- the finite-difference passes of the shaded backward.  OFF = 0 ignores both.  The kernels themselves are the templates, as
// k_ngp_field_bwd_mfma_t (ngp_bwd_mfma.h).
// The argument list and two pieces of text are kept as they were when the kernel was timed, because each shared form changes what hipcc
// emits for this kernel (profiles/ngp_scatter_refactor_regs.log, profiles/ngp_scatter_refactor_ab.log): one by-value struct moves its
// scalar loads and waits; ngp_z_dropped(lv, l) makes the run loop load lv.resolution[l] again for every sample; ngp_sample_x01 inside the
// run loop costs 6 VGPRs.  With positional arguments, the rule and the point written out, and sc_corner, it is the parent's code.
template <int NT, int OFF = 0>
SF_KERNEL(NT) void k_ngp_scatter(
    NgpLevels lv, float bound, long long* __restrict__ gtable, float* __restrict__ gtable_f, float thr, const float* __restrict__ rays_o,
    const float* __restrict__ rays_d, const float* __restrict__ aabb, const float* __restrict__ z_s,
    const float* __restrict__ dfeat, uint32_t N, uint32_t T2, uint32_t rays_per_row, uint32_t cached_levels,
    uint32_t last_level, uint32_t sc_run, uint32_t off_e, float off_eps) {
  SF_DYN_LDS(sc_lds);
  uint32_t* tags = reinterpret_cast<uint32_t*>(sc_lds);                                      // [SC_SLOTS]
  long long* vals = reinterpret_cast<long long*>(sc_lds + SC_SLOTS * sizeof(uint32_t));      // [SC_SLOTS][2], fixed point (sf_dev.h): exact, order-independent sums
  const uint32_t P = N * T2;
  float box[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) box[i] = aabb[i];
  // tile -> ray ids: 8x8 patch of the image if the layout is known, else 64 consecutive rays
  uint32_t tile_x = 0, tile_y = 0, tiles_x = 0;
  const bool patch = rays_per_row >= 8 && (rays_per_row % 8) == 0 && (N % rays_per_row) == 0 && ((N / rays_per_row) % 8) == 0;
  if (patch) { tiles_x = rays_per_row / 8; tile_y = blockIdx.x / tiles_x; tile_x = blockIdx.x % tiles_x; }

  for (uint32_t l = 0; l < last_level; ++l) {
    const bool cached = l < cached_levels;
    if (cached) {
      for (uint32_t s = threadIdx.x; s < SC_SLOTS; s += NT) { tags[s] = SC_EMPTY; vals[2 * s] = 0; vals[2 * s + 1] = 0; }
      sf_sync();
    }
    long long* tab = gtable + (size_t)lv.offset[l] * 2;
    float* ftab = gtable_f + (size_t)lv.offset[l] * 2;
    const uint32_t step = lv.resolution[l] + 1;                  // the rule of ngp_z_dropped (ngp_device.h), restated: see above
    const bool z_dropped = lv.gridtype == 1 && (uint64_t)step * step > lv.hsize[l] && step <= lv.hsize[l];
    // lane quads share a sample: lane&1 = channel, lane&2 = x-corner.  The four adds of an x-corner pair (two
    // adjacent table rows x 2 channels = 16 contiguous bytes) sit in adjacent lanes of ONE atomic instruction: the
    // memory-side atomic unit merges lanes of one granule (measured 13.5 -> 7.6 ms with channel pairs alone).
    // A thread-item = (ray, run of `sc_run` consecutive sorted samples, lane of the quad).  Consecutive samples of a ray share
    // their cell on the coarse levels, so equal rows are first summed in REGISTERS (run-length merge per corner pair) and
    // only the run totals go to the LDS cache: on levels 0-5 nearly every lane of every atomic instruction used to hit
    // the same handful of LDS addresses, and same-address LDS atomics serialise (0.18 ms per level for ~1 us of work).
    const uint32_t runs = (T2 + sc_run - 1) / sc_run;
    auto flush = [&](uint32_t row, float v, uint32_t ch) {
      if (!(fabsf(v) < thr)) {                                 // large / non-finite: the fp32 table (sf_grad_add)
        sf_global_add(ftab + (size_t)row * 2 + ch, v);
        return;
      }
      if (cached) {
        const uint32_t slot = (row * 2654435761u) >> 20;         // 12 bits -> SC_SLOTS
        const uint32_t prev = sf_atomic_cas_u32(&tags[slot], SC_EMPTY, row);
        if (prev == SC_EMPTY || prev == row) {
          sf_fix_add(&vals[2 * slot + ch], sf_fix_of(v));
          return;
        }
      }
      sf_fix_add(tab + (size_t)row * 2 + ch, sf_fix_of(v));      // (a slot held by another row: straight to the table)
    };
    for (uint32_t it = threadIdx.x; it < 4 * SC_RAYS * runs; it += NT) {
      const uint32_t q = it >> 2, ch = it & 1, xb = (it >> 1) & 1;
      const uint32_t r = q / runs, k0 = (q - r * runs) * sc_run;
      uint32_t n = patch ? ((tile_y * 8 + (r >> 3)) * rays_per_row + tile_x * 8 + (r & 7)) : (blockIdx.x * SC_RAYS + r);
      if (n >= N) continue;
      // The ray is loaded once per run and the point derived below in this kernel's own text, the steps of ngp_sample_x01
      // (ngp_point_attrs.h) restated: with the helper inside the run loop the kernel takes 82 / 84 VGPRs instead of 76 / 78.
      const float o[3] = {rays_o[n * 3], rays_o[n * 3 + 1], rays_o[n * 3 + 2]};
      const float d[3] = {rays_d[n * 3], rays_d[n * 3 + 1], rays_d[n * 3 + 2]};
      uint32_t prow[4] = {SC_EMPTY, SC_EMPTY, SC_EMPTY, SC_EMPTY};
      float pacc[4] = {0.f, 0.f, 0.f, 0.f};
      const uint32_t k1 = k0 + sc_run < T2 ? k0 + sc_run : T2;
      // (r04: the run walked in batches of 4 / 8 / 16 samples with their gradient and depth loads issued together measured SLOWER,
      // 3.76 / 3.76 / 3.86 against 3.55 ms render fwd + bwd, profiles/r04_ngp_binned_tuning.log: 128 VGPRs at 1024 threads, and the
      // kernel runs beside the last chunk's bin + reduce, whose memory traffic it then competes with)
      for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t p = n * T2 + k;
        const float dfc = dfeat[((size_t)l * P + p) * 2 + ch];
        if (dfc == 0.0f) continue;                               // outside points / dead samples contribute nothing
        float x[3], x01[3];
        ngp_point(o, d, z_s[p], box, x);
        if (OFF) {
          const float xc[3] = {x[0], x[1], x[2]};
          ngp_offset_point(xc, (int)off_e, off_eps, bound, x);
        }
        if (!ngp_unit(x, bound, x01)) continue;
        NgpCell c;
        ngp_cell(lv, l, x01, c);
#pragma unroll
        for (int yz = 0; yz < 4; ++yz) {
          if (z_dropped && yz >= 2) continue;
          uint32_t row;
          float w;
          sc_corner(c, z_dropped, yz, xb, row, w);
          const float v = SF_MUL(w, dfc);
          if (row == prow[yz]) {
            pacc[yz] += v;
          } else {
            if (prow[yz] != SC_EMPTY) flush(prow[yz], pacc[yz], ch);
            prow[yz] = row;
            pacc[yz] = v;
          }
        }
      }
#pragma unroll
      for (int yz = 0; yz < 4; ++yz)
        if (prow[yz] != SC_EMPTY) flush(prow[yz], pacc[yz], ch);
    }
    if (cached) {
      sf_sync();
      for (uint32_t s = threadIdx.x; s < SC_SLOTS; s += NT) {
        const uint32_t row = tags[s];
        if (row != SC_EMPTY) {
          if (vals[2 * s]) sf_fix_add(tab + (size_t)row * 2, vals[2 * s]);
          if (vals[2 * s + 1]) sf_fix_add(tab + (size_t)row * 2 + 1, vals[2 * s + 1]);
        }
      }
      sf_sync();
    }
  }
}

// Fine levels (cell smaller than the patch footprint: nothing to merge in LDS): no LDS frame, so 8 waves per SIMD hide the
// latency of the loads in front of every atomic.  Work item = (level, sample) in level-major order (the dfeat layout),
// lane quads as above: 16 contiguous bytes per atomic instruction and quad.
template <int OFF>
SF_KERNEL(256) void k_ngp_scatter_fine(SCArgs a) {
  const uint32_t P = a.N * a.T2;
  float box[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) box[i] = a.aabb[i];
  const uint64_t total = (uint64_t)4 * P * (a.lv.L - a.first_level);
  for (uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (uint64_t)gridDim.x * 256) {
    const uint32_t ch = (uint32_t)it & 1, xb = ((uint32_t)it >> 1) & 1;
    const uint64_t q = it >> 2;
    const uint32_t l = a.first_level + (uint32_t)(q / P), p = (uint32_t)(q % P);
    const float dfc = a.dfeat[((size_t)l * a.P_stride + a.p_off + p) * 2 + ch];
    if (dfc == 0.0f) continue;
    float x[3], x01[3];
    if (!ngp_sample_x01<OFF>(a.rays_o, a.rays_d, p / a.T2, a.z_s[p], box, a.bound, a.off_e, a.off_eps, x, x01)) continue;
    NgpCell c;
    ngp_cell(a.lv, l, x01, c);
    long long* tab = a.gtable + (size_t)a.lv.offset[l] * 2;
    float* ftab = a.gtable_f + (size_t)a.lv.offset[l] * 2;
    const bool z_dropped = ngp_z_dropped(a.lv, l);
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
      if (z_dropped && yz >= 2) continue;
      uint32_t row;
      float w;
      sc_corner(c, z_dropped, yz, xb, row, w);
      sf_grad_add(tab + (size_t)row * 2 + ch, ftab + (size_t)row * 2 + ch, SF_MUL(w, dfc), a.thr);
    }
  }
}

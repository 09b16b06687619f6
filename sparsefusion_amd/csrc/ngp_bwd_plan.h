// Host-side plan of sf_ngp_render_backward (ngp_render.hip): ray chunks, the launch geometry of the field backward, the level split of the
// table-gradient scatter and the workspace sizes.  Plain C++ over NgpLevels: no HIP type, nothing launched, so a host compiler builds it
// and tests/hostemu/ngp_bwd_emu.cpp exports it to tests/test_hostemu_ngp_bwd.py as it stands.
#pragma once
#include "ngp_device.h"                            // NgpLevels, NGP_MAX_LEVELS
#include "sf_fix.h"                                // sf_fix_thr

// buckets of the binned scatter (ngp_scatter_bin.h)
#ifndef SB_ROWS_LOG
#define SB_ROWS_LOG 10          // measured on the reference field (2^16-row `tiled` levels), render fwd + bwd: 2048 / 1024 / 512 rows = 4.27 / 3.90 / 4.13 ms
#endif
#define SB_ROWS (1u << SB_ROWS_LOG)   // table rows per bucket
static_assert(SB_ROWS_LOG <= 10, "the entry word keeps row1 - row0 + 1024 in 11 bits");
#define SB_MAX_BUCKETS (1u << (19 - SB_ROWS_LOG))            // per level: hsize <= 2^19, the reference's log2_hashmap_size (larger tables keep k_ngp_scatter_fine)

// the backward cuts the rays into chunks (the pipeline of sf_ngp_render_backward): as many as keep a chunk a multiple of 256 rays and >= 2048 rays
#ifndef NGP_BWD_CHUNKS
#define NGP_BWD_CHUNKS 2u       // r03 (atomic scatters): 1 / 2 / 4 / 8 chunks = 5.96 / 5.65 / 5.64 / 6.00 ms; r04 (binned): 1 / 2 / 4 / 8 = 3.71 / 3.55 / 3.68 / 4.11 ms
#endif
struct NgpChunks { uint32_t n, max_rays, start[66]; };      // chunk c = rays [start[c], start[c + 1])
static inline NgpChunks ngp_bwd_plan(uint32_t N) {
  NgpChunks c{};
  auto equal = [&](uint32_t k) {
    c.n = k; c.max_rays = N / k;
    for (uint32_t i = 0; i <= k; ++i) c.start[i] = i * (N / k);
  };
  auto ok = [&](uint32_t rays, uint32_t k) { return k >= 1 && rays % k == 0 && (rays / k) % 256 == 0 && rays / k >= 2048; };
  // (a small first chunk, so that the side stream starts early, measured slower: first chunk 1/4, 1/8, 1/16 of the rays = 3.63 / 3.63 /
  // 3.66 ms against 3.54 for two equal chunks, profiles/r04_ngp_binned_tuning.log -- co-running kernels cost their sum, not their maximum)
  // large ray sets: chunks of at most 8192 rays, so that the bins of one chunk (the workspace) stay at 1.6 GB
  for (uint32_t k = (N + 8191) / 8192; k > NGP_BWD_CHUNKS && k <= 64; ++k)
    if (ok(N, k)) { equal(k); return c; }
  uint32_t k = NGP_BWD_CHUNKS;
  while (k > 1 && !ok(N, k)) --k;
  if (N / k > 8192) {                   // (r06, ADVICE r05: also when an equal split exists but is coarser than 8192 rays -- N = 51 712 = 2 x 25 856)
    // r05: a ray count with no equal split (N = 200^2, 65 535, ...) used to fall back to ONE chunk, and the bins -- sized by
    // the largest chunk -- then grew with all rays (7.9 GB at 40 000 rays, 13 GB at 65 535).  Unequal chunks: as many chunks of `per`
    // rays (a multiple of 256, 8192 unless that needs more than 64 chunks) as fit, and the remainder as the last one; the kernels take
    // any (offset, count) -- only the bins' size depends on max_rays.
    uint32_t per = 8192;
    if ((N + per - 1) / per > 64) per = (((N + 63) / 64 + 255) / 256) * 256;
    c.n = (N + per - 1) / per; c.max_rays = per;
    for (uint32_t i = 0; i < c.n; ++i) c.start[i] = i * per;
    c.start[c.n] = N;
    return c;
  }
  equal(k);
  return c;
}
// all rays as one chunk: a backward with nothing to run beside the field backward (no table gradient, or every level in k_ngp_scatter)
static inline NgpChunks ngp_bwd_one_chunk(uint32_t N) {
  NgpChunks c{};
  c.n = 1; c.max_rays = N; c.start[1] = N;
  return c;
}

// Field backward (k_ngp_field_bwd_mfma / k_ngp_field_bwd_pipe) over the P points of one chunk, `pts` points per wave and trip.
static inline uint32_t ngp_field_bwd_grid(uint32_t P, uint32_t pts) {
  auto sf_div_up = [](uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); };      // (sf_common.h's, which needs the HIP runtime)
  const uint32_t trips = sf_div_up(P, pts);
  const uint32_t grid = trips < 1024 ? sf_div_up(trips, 4) : 256;   // one resident workgroup per CU (LDS-bound), 4 waves each
  return grid;
}
// Fixed-point threshold of the MLP gradients.
static inline float ngp_bwd_thr_mlp(uint32_t n_chunks) {
  return sf_fix_thr(4.0 * 256.0 * n_chunks);        // one addend per wave and launch: <= 256 workgroups x 4 waves per chunk
}

// workspace (floats): forward z_c, sig_c [N*T]; rgb_c [3NT]; z_f, sig_f [N*T]; rgb_f [3NT]  -> 10*N*T
// backward: dsig [2NT] + drgb [6NT] + d(features) level-major [16][2NT][2] = 72*N*T, then the binned scatter's cursors and entries.
// binned scatter (ngp_scatter_bin.h): cursors + 16-byte entries of ONE chunk: 4 corner pairs x every level + slack per bucket
#define SB_CURSOR_WORDS (NGP_MAX_LEVELS * SB_MAX_BUCKETS)
#ifndef SB_LEVELS_BUDGET
#define SB_LEVELS_BUDGET 24                       // entries for 24 level-slots per sample (12 levels are binned): a bucket holds 2 x its uniform
#endif                                            // share (max / mean of the bucket loads on the reference scene: <= 1.9; 16 / 24 / 32 slots: 3.61 / 3.55 / 3.58 ms)
static inline uint64_t ngp_bin_entries(uint32_t N, uint32_t T) {
  return (uint64_t)ngp_bwd_plan(N).max_rays * 2 * T * 4 * SB_LEVELS_BUDGET + (uint64_t)SB_CURSOR_WORDS * 64;
}
static inline uint64_t ngp_bwd_grad_floats(uint32_t N, uint32_t T) { return (uint64_t)(8 + 4 * NGP_MAX_LEVELS) * N * T; }      // dsig | drgb | d(features)
static inline uint64_t ngp_render_workspace_bytes(uint32_t N, uint32_t T) {
  return ngp_bwd_grad_floats(N, T) * sizeof(float) + (uint64_t)SB_CURSOR_WORDS * 4 + ngp_bin_entries(N, T) * 16;
}
static inline uint64_t ngp_render_forward_workspace_bytes(uint32_t N, uint32_t T) { return (uint64_t)10 * N * T * sizeof(float); }

// Which kernel scatters which level of the table gradient: levels [0, last) go to k_ngp_scatter (ngp_scatter.h), [0, cached) of them through
// its LDS cache; levels [last, L) go to the binned scatter (binned; ngp_scatter_bin.h) or to k_ngp_scatter_fine (ngp_scatter.h), chunk by chunk.  bucket0[l]: first bucket of level l,
// total_buckets of bin_cap entries each.
struct NgpScatterPlan {
  uint32_t cached, first_bin, last, total_buckets, bin_cap;
  bool binned;
  uint32_t bucket0[NGP_MAX_LEVELS + 1];
};
static inline NgpScatterPlan ngp_scatter_plan(const NgpLevels& lv, bool table_grad, uint32_t N, uint32_t T) {
  NgpScatterPlan s{};
  // scatter shape, measured on MI355X in r02 (the A/B environment switches were retired in r04): 1024 threads per cached-level
  // workgroup (256 / 512 / 1024: 8.55 / - / 7.84 ms render fwd+bwd), LDS cache up to scale 640 (160 / 320 / 640 / all levels: 7.82 /
  // 7.63 / 7.51 / 8.27 ms), the finer levels in their own high-occupancy launch, 32 sorted samples merged per thread before the cache
  // (4 / 8 / 16 / 32: 6.95 / 6.85 / 6.81 / 6.76 ms)
  constexpr float sc_cutoff = 640.0f;
  // levels up to scale ~640 profit from the LDS cache (measured r02: cut-off 160 / 320 / 640 / none = 7.82 / 7.63 / 7.51 / 8.27 ms render fwd+bwd)
  uint32_t cached = 0;
  while (cached < lv.L && lv.scale[cached] <= sc_cutoff) ++cached;
  // r04: the levels whose cell is smaller than a ray patch's footprint (no merging in the LDS cache) are BINNED by table slice and
  // reduced in LDS instead of sending one device atomic per corner (ngp_scatter_bin.h); tables beyond 2^22 rows keep the atomics
  // (measured r04, render fwd + bwd: atomics 5.02 ms; binned from scale > 45 / 60 / 80 / 112 / 160: 4.97 / 4.45 / 4.50 / 4.43 / 4.58 ms with
  // one entry per corner, 60 / 112: 4.20 / 4.21 ms with pair entries, profiles/r04_ngp_binned_scatter_ab.log; the A/B switches are
  // retired: the dense levels keep the LDS cache, the hashed ones are binned)
  constexpr float bin_cutoff = 60.0f;
  uint32_t first_bin = lv.L;
  if (table_grad) {
    first_bin = 0;
    while (first_bin < lv.L && lv.scale[first_bin] <= bin_cutoff) ++first_bin;
    uint32_t tb = 0;
    for (uint32_t l = 0; l <= NGP_MAX_LEVELS; ++l) {
      s.bucket0[l] = tb;
      if (l >= first_bin && l < lv.L) {
        const uint32_t nb = (lv.hsize[l] + SB_ROWS - 1) >> SB_ROWS_LOG;
        if (nb > SB_MAX_BUCKETS) { first_bin = lv.L; break; }
        tb += nb;
      }
    }
  }
  const bool binned = first_bin < lv.L;
  if (binned && cached > first_bin) cached = first_bin;
  const uint32_t last = !table_grad ? lv.L : binned ? first_bin : cached;     // levels [0, last): k_ngp_scatter, [last, L): binned / k_ngp_scatter_fine
  s.cached = cached; s.first_bin = first_bin; s.binned = binned; s.last = last;
  s.total_buckets = s.bucket0[NGP_MAX_LEVELS];
  s.bin_cap = binned ? (uint32_t)(ngp_bin_entries(N, T) / s.total_buckets) : 0;
  return s;
}

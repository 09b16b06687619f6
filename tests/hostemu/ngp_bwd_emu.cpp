// CPU harness for the MFMA field-backward kernel (sparsefusion_amd/csrc/ngp_bwd_mfma.h): the kernel source runs on CPU
// threads (hip_emu.h) and is compared by tests/test_hostemu_ngp_bwd.py with the per-point reference math of
// ngp_device.h (ngp_mlp_forward / ngp_mlp_backward, the functions the oracle-checked host emulation uses).
#ifndef SF_HOST_EMU
#define SF_HOST_EMU
#endif
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"
#define NGP_EMU_FIELD_BWD
#include "ngp_emu_common.h"
#include "../../sparsefusion_amd/csrc/ngp_bwd_plan.h"

extern "C" void emu_field_bwd(const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                              const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                              float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* z_s,
                              const float* dsig, const float* drgb, uint32_t P, uint32_t T2, uint32_t grid, int use_ref,
                              float* g_w0, float* g_b0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* dfeat) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  if (use_ref != 1) {
    // use_ref == 2: the kernel on a field cache (features + permutation as the forward would leave them) instead of the re-gather
    EmuFieldCache cache;
    if (use_ref == 2) {
      std::vector<float> feat((size_t)P * NGP_FEAT);
      emu_encode_points(lv, table, bound, rays_o, rays_d, aabb, z_s, P, T2, feat.data(), nullptr, nullptr);
      cache.build(feat.data(), P, T2);
    }
    EmuFixAcc acc(g_w0, g_b0, g_w1, g_b1, g_w2, g_b2);
    // thr: one addend per wave, as the product's bound
    FBArgs a = emu_fb_args(lv, table, w0, b0, w1, b1, w2, b2, bound, acc, sf_fix_thr(4.0 * grid), rays_o, rays_d, aabb, z_s, dsig, drgb, dfeat, 0,
                           P / T2, T2, P, use_ref == 2 ? &cache : nullptr);
    a.P = P;
    hipemu::launch(grid, 256, FB_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_bwd_mfma(a); });
    acc.convert();
    return;
  }
  // reference: per-point math (ngp_device.h), serial
  std::vector<float> W;
  pack_weights(W, w0, b0, w1, b1, w2, b2);
  for (uint32_t p = 0; p < P; ++p) {
    const uint32_t n = p / T2;
    float x[3], x01[3], feat[NGP_FEAT], h1[NGP_HID], h2[NGP_HID], out[NGP_OUT], dout[NGP_OUT];
    const bool inside = ngp_sample_x01<0>(rays_o, rays_d, n, z_s[p], aabb, bound, 0, 0.0f, x, x01);
    ngp_encode(lv, table, x01, inside, feat);
    ngp_mlp_forward(W.data(), feat, h1, h2, out);
    const float pre = out[0] + ngp_blob(x);
    dout[0] = dsig[p] * expf(fminf(fmaxf(pre, -15.0f), 15.0f));
    for (int c = 0; c < 3; ++c) { const float s = ngp_sigmoid(out[1 + c]); dout[1 + c] = drgb[p * 3 + c] * s * (1.0f - s); }
    float dh2[NGP_HID], dh1[NGP_HID], df[NGP_FEAT];
    ngp_mlp_backward(W.data(), h1, h2, dout, dh2, dh1, df);
    for (int j = 0; j < NGP_OUT; ++j) { g_b2[j] += dout[j]; for (int k = 0; k < NGP_HID; ++k) g_w2[j * NGP_HID + k] += dout[j] * h2[k]; }
    for (int j = 0; j < NGP_HID; ++j) { g_b1[j] += dh2[j]; for (int k = 0; k < NGP_HID; ++k) g_w1[j * NGP_HID + k] += dh2[j] * h1[k]; }
    for (int j = 0; j < NGP_HID; ++j) { g_b0[j] += dh1[j]; for (int k = 0; k < NGP_FEAT; ++k) g_w0[j * NGP_FEAT + k] += dh1[j] * feat[k]; }
    for (uint32_t l = 0; l < L; ++l) {
      dfeat[((size_t)l * P + p) * 2] = inside ? df[2 * l] : 0.0f;
      dfeat[((size_t)l * P + p) * 2 + 1] = inside ? df[2 * l + 1] : 0.0f;
    }
  }
}

// ---- the per-element float64 checks of tests/ngp_bwd_cases.py: the features ngp_encode gives every point (the values the kernel's re-gather
// loop computes, and what a field cache holds), and the kernel launched chunk by chunk the way sf_ngp_render_backward does -- ray / sample
// pointers offset to the chunk, d(feat) in the layout of the whole set (dfeat_P, p_off), one thr for all launches, any grid per chunk
extern "C" void emu_features(const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype, float bound,
                             const float* rays_o, const float* rays_d, const float* aabb, const float* z_s, uint32_t P, uint32_t T2,
                             float* feat, float* xyz, float* inside_out) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  emu_encode_points(lv, table, bound, rays_o, rays_d, aabb, z_s, P, T2, feat, xyz, inside_out);
}

extern "C" void emu_field_bwd_chunks(const float* table, const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                     const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                                     float bound, const float* rays_o, const float* rays_d, const float* aabb, const float* z_s,
                                     const float* dsig, const float* drgb, uint32_t N, uint32_t T2, uint32_t n_chunks, const uint32_t* start,
                                     const uint32_t* grids, float thr, const float* feat_sorted,
                                     float* g_w0, float* g_b0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* dfeat) {
  const uint32_t P = N * T2;
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  EmuFieldCache cache;
  if (feat_sorted) cache.build(feat_sorted, P, T2);            // a field cache holding the given rows
  EmuFixAcc acc(g_w0, g_b0, g_w1, g_b1, g_w2, g_b2);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const FBArgs a = emu_fb_args(lv, table, w0, b0, w1, b1, w2, b2, bound, acc, thr, rays_o, rays_d, aabb, z_s, dsig, drgb, dfeat, start[c],
                                 start[c + 1] - start[c], T2, P, feat_sorted ? &cache : nullptr);
    hipemu::launch(grids[c], 256, FB_LDS_FLOATS * sizeof(float), [&] { k_ngp_field_bwd_mfma(a); });
  }
  acc.convert();
}

// ---- the host plan of sf_ngp_render_backward (sparsefusion_amd/csrc/ngp_bwd_plan.h) as the product calls it, for the restatement of
// tests/ngp_bwd_cases.py.  start: room for 66 words.  emu_scatter_plan's out: cached, first_bin, binned, last, total_buckets, bin_cap,
// then bucket0[NGP_MAX_LEVELS + 1].
extern "C" void emu_bwd_plan(uint32_t N, uint32_t* n, uint32_t* max_rays, uint32_t* start) {
  const NgpChunks c = ngp_bwd_plan(N);
  *n = c.n; *max_rays = c.max_rays;
  for (uint32_t i = 0; i < 66; ++i) start[i] = c.start[i];
}
extern "C" uint32_t emu_field_bwd_grid(uint32_t P) { return ngp_field_bwd_grid(P, FB_PTS); }
extern "C" float emu_bwd_thr_mlp(uint32_t n_chunks) { return ngp_bwd_thr_mlp(n_chunks); }
extern "C" void emu_scatter_plan(const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype, int table_grad, uint32_t N,
                                 uint32_t T, uint32_t* out) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  const NgpScatterPlan s = ngp_scatter_plan(lv, table_grad != 0, N, T);
  const uint32_t head[6] = {s.cached, s.first_bin, s.binned ? 1u : 0u, s.last, s.total_buckets, s.bin_cap};
  for (int i = 0; i < 6; ++i) out[i] = head[i];
  for (uint32_t l = 0; l <= NGP_MAX_LEVELS; ++l) out[6 + l] = s.bucket0[l];
}

// ---- binned table-gradient scatter (sparsefusion_amd/csrc/ngp_scatter_bin.h) against ngp_scatter (ngp_device.h), levels
// [first_level, L); `chunks` rounds of bin + reduce over consecutive ray ranges share the entries buffer (cursor reset by the reducer)
#include "../../sparsefusion_amd/csrc/ngp_scatter_bin.h"
extern "C" int emu_bin_scatter(const int32_t* h_offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype, float bound,
                               const float* rays_o, const float* rays_d, const float* aabb, const float* z_s, const float* dfeat,
                               uint32_t N, uint32_t T2, uint32_t first_level, uint32_t cap, uint32_t chunks, uint32_t grid, int use_ref,
                               float* gtable) {
  NgpLevels lv;
  fill_levels(&lv, h_offsets, L, S, H, gridtype);
  const uint32_t P = N * T2;
  if (use_ref) {
    for (uint32_t p = 0; p < P; ++p) {
      const uint32_t n = p / T2;
      float x[3], x01[3], df[NGP_FEAT] = {0};
      const bool inside = ngp_sample_x01<0>(rays_o, rays_d, n, z_s[p], aabb, bound, 0, 0.0f, x, x01);
      for (uint32_t l = first_level; l < L; ++l) { df[2 * l] = dfeat[((size_t)l * P + p) * 2]; df[2 * l + 1] = dfeat[((size_t)l * P + p) * 2 + 1]; }
      ngp_scatter(lv, gtable, x01, inside, df);
    }
    return 0;
  }
  SBArgs b{};
  SBRArgs r{};
  uint32_t tb = 0;
  for (uint32_t l = 0; l <= NGP_MAX_LEVELS; ++l) {
    b.bucket0[l] = r.bucket0[l] = tb;
    if (l >= first_level && l < L) {
      const uint32_t nb = (lv.hsize[l] + SB_ROWS - 1) >> SB_ROWS_LOG;
      if (nb > SB_MAX_BUCKETS) return 1;
      tb += nb;
    }
  }
  std::vector<uint32_t> cursor(tb, 0);
  std::vector<f32x4> ent((size_t)tb * cap);
  std::vector<long long> gacc((size_t)h_offsets[L] * 2, 0);           // fixed-point sums (sf_dev.h), added to gtable at the end
  b.lv = lv; b.bound = bound; b.aabb = aabb; b.dfeat = dfeat; b.gtable = gacc.data(); b.gtable_f = gtable; b.thr = sf_fix_thr(8.0 * P); b.cursor = cursor.data(); b.ent = ent.data();
  b.T2 = T2; b.first_level = first_level; b.P_stride = P; b.cap = cap;
  r.lv = lv; r.gtable = gacc.data(); r.gtable_f = gtable; r.thr = b.thr; r.cursor = cursor.data(); r.ent = ent.data(); r.first_level = first_level; r.cap = cap;
  const uint32_t Nc = (N + chunks - 1) / chunks;
  for (uint32_t c = 0; c * Nc < N; ++c) {
    const uint32_t n0 = c * Nc, nn = n0 + Nc <= N ? Nc : N - n0;
    b.rays_o = rays_o + (size_t)n0 * 3; b.rays_d = rays_d + (size_t)n0 * 3; b.z_s = z_s + (size_t)n0 * T2; b.P = nn * T2; b.p_off = n0 * T2;
    hipemu::launch(grid, SB_THREADS, 0, [&] { k_ngp_bin(b); });
    hipemu::launch(tb, SBR_THREADS, 0, [&] { k_ngp_bin_reduce(r); });
    for (uint32_t k = 0; k < tb; ++k) if (cursor[k]) return 2;          // the reducer leaves every cursor at zero
  }
  for (size_t i = 0; i < gacc.size(); ++i) gtable[i] += (float)((double)gacc[i] * SF_FIX_INV);
  return 0;
}

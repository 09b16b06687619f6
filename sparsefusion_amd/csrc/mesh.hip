// Mesh export (NeRFRenderer.export_mesh, external/nerf/renderer_df.py:122-165; extract_fields / extract_geometry,
// external/nerf/utils.py:174-204): the NGP density on a lattice, the separable Gaussian + volume statistics and marching cubes
// of mesh_kernels.h, the point attributes of ngp_point_attrs.h and the texture bake of ngp_texture.h (the reference's _export,
// renderer_df.py:166-306), and the connected components / floater removal of mesh_clean.h (no counterpart in the reference, which
// leaves clean-up to pymeshlab).  Host entry points declared in include/sparsefusion_hip.h.  See DESIGN.md section 9.
#include "sf_common.h"
#include "mesh_kernels.h"
#include "mesh_clean.h"
#include "ngp_field_lds.h"
#include "ngp_point_attrs.h"
#include "ngp_texture.h"

// sigma at (ax[i], ay[j], az[k]) -> sigma[(i * ny + j) * nz + k], straight from the lattice index (no point buffer).  The per-point
// code is k_ngp_field's (ngp_render.hip): weights in LDS, the same encode / MLP / activation, so a lattice value is bit-identical
// to sf_ngp_density on the same fp32 point.  The barrier at the top of each round of the grid-stride loop keeps the compiler
// from hoisting the loop-invariant LDS weight reads out of the loop (which would pin them in registers and spill).
__global__ __launch_bounds__(256) void k_ngp_lattice(FieldPtrs f, NgpLevels lv, const float* __restrict__ ax, const float* __restrict__ ay,
                                                     const float* __restrict__ az, uint32_t nx, uint32_t ny, uint32_t nz,
                                                     float* __restrict__ sigma) {
  __shared__ __attribute__((aligned(16))) float W[NGP_WTOTAL];
  load_weights_lds(W, f);
  const uint64_t P = (uint64_t)nx * ny * nz;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < P; base += (uint64_t)gridDim.x * blockDim.x) {
    __syncthreads();
    const uint64_t p = base + threadIdx.x;
    if (p >= P) continue;
    const uint32_t k = (uint32_t)(p % nz), j = (uint32_t)((p / nz) % ny), i = (uint32_t)(p / ((uint64_t)ny * nz));
    const float x[3] = {ax[i], ay[j], az[k]};
    float x01[3];
    const bool inside = ngp_unit(x, f.bound, x01);
    float feat[NGP_FEAT], h1[NGP_HID], h2[NGP_HID], out[NGP_OUT];
    ngp_encode(lv, f.table, x01, inside, feat);
    ngp_mlp_forward(W, feat, h1, h2, out);
    sigma[p] = expf(out[0] + ngp_blob(x));
  }
}

static bool mesh_dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && (uint64_t)nx * ny * nz < (1ull << 31);
}

extern "C" int sf_ngp_density_lattice(const sf_ngp_field* f, const float* ax, const float* ay, const float* az, uint32_t nx,
                                      uint32_t ny, uint32_t nz, float* sigma, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!mesh_dims_ok(nx, ny, nz)) SF_FAIL(SF_ERR_INVALID, "ngp_density_lattice: need 1 <= nx, ny, nz and nx*ny*nz < 2^31");
  if (!ax || !ay || !az || !sigma) SF_FAIL(SF_ERR_INVALID, "ngp_density_lattice: null pointer");
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  k_ngp_lattice<<<sf_grid_cap(sf_div_up((uint64_t)nx * ny * nz, 256)), 256, 0, st>>>(sf_ngp_field_ptrs(f), lv, ax, ay, az, nx, ny, nz,
                                                                                    sigma);
  SF_CHECK_LAUNCH("ngp_density_lattice");
  return SF_OK;
}

// sigma, albedo, finite-difference gradient and normal at P points (ngp_point_attrs.h): seven evaluations of the field per thread,
// one after the other, each bit-identical to sf_ngp_density on its fp32 point.  Launch shape, LDS weights and the barrier at the
// top of each round as k_ngp_lattice.  Null outputs are skipped; with neither grad nor normal only the centre is evaluated.
__global__ __launch_bounds__(256) void k_ngp_point_attrs(FieldPtrs f, NgpLevels lv, const float* __restrict__ xyz, uint32_t P, float eps,
                                                         float* __restrict__ sigma, float* __restrict__ albedo, float* __restrict__ grad,
                                                         float* __restrict__ normal) {
  __shared__ __attribute__((aligned(16))) float W[NGP_WTOTAL];
  load_weights_lds(W, f);
  const int n_eval = (grad || normal) ? 7 : 1;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < P; base += (uint64_t)gridDim.x * blockDim.x) {
    __syncthreads();
    const uint64_t p = base + threadIdx.x;
    if (p >= P) continue;
    const float x[3] = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
    NgpPointAttrs a;
    ngp_point_attrs(lv, f.table, W, f.bound, x, eps, n_eval, a);
    if (sigma) sigma[p] = a.sigma;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (albedo) albedo[3 * p + c] = a.albedo[c];
      if (grad) grad[3 * p + c] = a.grad[c];
      if (normal) normal[3 * p + c] = a.normal[c];
    }
  }
}

extern "C" int sf_ngp_point_attrs(const sf_ngp_field* f, const float* xyz, uint32_t P, float epsilon, float* sigma, float* albedo,
                                  float* grad, float* normal, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!f || !xyz) SF_FAIL(SF_ERR_INVALID, "ngp_point_attrs: null field or points");
  if (!sigma && !albedo && !grad && !normal) SF_FAIL(SF_ERR_INVALID, "ngp_point_attrs: at least one output is required");
  if (!isfinite(epsilon) || !(epsilon > 0.0f)) SF_FAIL(SF_ERR_INVALID, "ngp_point_attrs: epsilon must be finite and > 0");
  if (P == 0) return SF_OK;
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  k_ngp_point_attrs<<<sf_grid_cap(sf_div_up(P, 256)), 256, 0, st>>>(sf_ngp_field_ptrs(f), lv, xyz, P, epsilon, sigma, albedo, grad, normal);
  SF_CHECK_LAUNCH("ngp_point_attrs");
  return SF_OK;
}

// Texture atlas of a mesh baked from the field (ngp_texture.h): one thread per texel -- its face and clamped barycentrics from the
// texel index, the point on the face, one evaluation of the field (bit-identical to sf_ngp_density on that fp32 point), the stores.
// Launch shape, LDS weights and the barrier at the top of each round as k_ngp_lattice.  Null outputs are skipped.
__global__ __launch_bounds__(256) void k_ngp_texture_bake(FieldPtrs f, NgpLevels lv, NgpAtlas at, const float* __restrict__ verts,
                                                          uint32_t V, const int32_t* __restrict__ faces, uint32_t F, NgpTexOut o) {
  __shared__ __attribute__((aligned(16))) float W[NGP_WTOTAL];
  load_weights_lds(W, f);
  const uint64_t P = (uint64_t)at.W * at.W;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < P; base += (uint64_t)gridDim.x * blockDim.x) {
    __syncthreads();
    const uint64_t t = base + threadIdx.x;
    if (t >= P) continue;
    ngp_texture_texel(lv, f.table, W, f.bound, at, verts, V, faces, F, (uint32_t)t, o);
  }
}

extern "C" int sf_ngp_texture_bake(const sf_ngp_field* f, const float* verts, uint32_t V, const int32_t* faces, uint32_t F, uint32_t W,
                                   uint8_t* rgb8, float* albedo, float* xyz, int32_t* face_id, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!f || !verts || !faces) SF_FAIL(SF_ERR_INVALID, "ngp_texture_bake: null field, vertices or faces");
  if (!rgb8 && !albedo && !xyz && !face_id) SF_FAIL(SF_ERR_INVALID, "ngp_texture_bake: at least one output is required");
  NgpAtlas at;
  switch (ngp_atlas_make(F, W, &at)) {
    case 1: SF_FAIL(SF_ERR_INVALID, "ngp_texture_bake: W must be >= 1");
    case 2: SF_FAIL(SF_ERR_INVALID, "ngp_texture_bake: need W * W < 2^31");
    case 3: SF_FAIL(SF_ERR_INVALID, "ngp_texture_bake: %u faces in a %u x %u texture leave cells of %u texels, below 6: the smallest W is %u",
                    F, W, W, at.c, 6 * at.G);
    default: break;
  }
  NgpLevels lv;
  if (int rc = sf_ngp_make_levels(f, &lv, st)) return rc;
  k_ngp_texture_bake<<<sf_grid_cap(sf_div_up((uint64_t)W * W, 256)), 256, 0, st>>>(sf_ngp_field_ptrs(f), lv, at, verts, V, faces, F,
                                                                                 NgpTexOut{rgb8, albedo, xyz, face_id});
  SF_CHECK_LAUNCH("ngp_texture_bake");
  return SF_OK;
}

// ----------------------------------------------------------------------------------------------------------------- Gaussian
static uint64_t align256(uint64_t b) { return (b + 255) & ~255ull; }

static uint32_t gauss_stat_wgs(uint32_t nx, uint32_t ny, uint32_t nz) {
  const uint64_t tiles = (uint64_t)nx * ny * sf_div_up(nz, GS_NT);
  return (uint32_t)(tiles < GS_STAT_WG ? tiles : GS_STAT_WG);
}

extern "C" uint64_t sf_gaussian3d_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
  if (!mesh_dims_ok(nx, ny, nz)) return 0;
  return align256((uint64_t)nx * ny * nz * sizeof(float)) + align256((uint64_t)gauss_stat_wgs(nx, ny, nz) * 2 * sizeof(double));
}

extern "C" int sf_gaussian3d(const float* in, float* out, uint32_t nx, uint32_t ny, uint32_t nz, float sigma, float truncate,
                             double* stats, void* ws, uint64_t ws_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!mesh_dims_ok(nx, ny, nz)) SF_FAIL(SF_ERR_INVALID, "gaussian3d: need 1 <= nx, ny, nz and nx*ny*nz < 2^31");
  if (!in || !out || !ws) SF_FAIL(SF_ERR_INVALID, "gaussian3d: null pointer");
  if (in == out) SF_FAIL(SF_ERR_INVALID, "gaussian3d: in and out must not alias");
  if (ws_bytes < sf_gaussian3d_workspace_bytes(nx, ny, nz)) SF_FAIL(SF_ERR_INVALID, "gaussian3d: workspace too small");
  GaussTaps taps;
  if (!gs_make_taps(sigma, truncate, &taps))
    SF_FAIL(SF_ERR_INVALID, "gaussian3d: need sigma > 0, truncate >= 0 and radius int(truncate * sigma + 0.5) <= %d", GS_RMAX);
  float* tmp = (float*)ws;
  double* partial = (double*)((char*)ws + align256((uint64_t)nx * ny * nz * sizeof(float)));
  const uint32_t segx = sf_div_up(nx, GS_SEG), segy = sf_div_up(ny, GS_SEG);
  k_gauss_strided<<<sf_div_up((uint64_t)segx * ny * nz, GS_NT), GS_NT, 0, st>>>(in, out, 1, nx, ny * nz, taps);       // axis 0
  SF_CHECK_LAUNCH("gaussian3d axis 0");
  k_gauss_strided<<<sf_div_up((uint64_t)nx * segy * nz, GS_NT), GS_NT, 0, st>>>(out, tmp, nx, ny, nz, taps);          // axis 1
  SF_CHECK_LAUNCH("gaussian3d axis 1");
  const uint32_t nwg = gauss_stat_wgs(nx, ny, nz);
  k_gauss_rows<<<nwg, GS_NT, 0, st>>>(tmp, out, (uint64_t)nx * ny, nz, taps, stats ? partial : nullptr);             // axis 2
  SF_CHECK_LAUNCH("gaussian3d axis 2");
  if (stats) {
    k_gauss_stats<<<1, GS_NT, 0, st>>>(partial, nwg, (uint64_t)nx * ny * nz, stats);
    SF_CHECK_LAUNCH("gaussian3d stats");
  }
  return SF_OK;
}

// ----------------------------------------------------------------------------------------------------------- marching cubes
// Workspace: code u16 [N] | vbase u32 [N] | bsum u32 [2 * nblk] | boff u32 [2 * nblk]
struct McWs { uint16_t* code; uint32_t* vbase; uint32_t* bsum; uint32_t* boff; };

static uint32_t mc_blocks(uint32_t nx, uint32_t ny, uint32_t nz) { return sf_div_up((uint64_t)nx * ny * nz, MC_BLOCK); }

// V <= 3 N and F <= 5 cells: both must fit in int32 before anything runs (nothing is read back)
static bool mc_dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
  if (!mesh_dims_ok(nx, ny, nz)) return false;
  const uint64_t N = (uint64_t)nx * ny * nz, cells = (uint64_t)(nx - 1) * (ny - 1) * (nz - 1);
  return 3 * N < (1ull << 31) && 5 * cells < (1ull << 31);
}

static McWs mc_ws(void* ws, uint32_t nx, uint32_t ny, uint32_t nz) {
  const uint64_t N = (uint64_t)nx * ny * nz, nb = mc_blocks(nx, ny, nz);
  char* b = (char*)ws;
  McWs w;
  w.code = (uint16_t*)b;
  b += align256(N * 2);
  w.vbase = (uint32_t*)b;
  b += align256(N * 4);
  w.bsum = (uint32_t*)b;
  b += align256(nb * 8);
  w.boff = (uint32_t*)b;
  return w;
}

extern "C" uint64_t sf_mc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
  if (!mc_dims_ok(nx, ny, nz)) return 0;
  const uint64_t N = (uint64_t)nx * ny * nz, nb = mc_blocks(nx, ny, nz);
  return align256(N * 2) + align256(N * 4) + 2 * align256(nb * 8);
}

static int mc_check(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, void* ws, uint64_t ws_bytes, const char* what) {
  if (!mc_dims_ok(nx, ny, nz)) SF_FAIL(SF_ERR_INVALID, "%s: need 1 <= nx, ny, nz, 3*nx*ny*nz < 2^31 and 5*(nx-1)*(ny-1)*(nz-1) < 2^31", what);
  if (!vol || !ws) SF_FAIL(SF_ERR_INVALID, "%s: null pointer", what);
  if (ws_bytes < sf_mc_workspace_bytes(nx, ny, nz)) SF_FAIL(SF_ERR_INVALID, "%s: workspace too small", what);
  return SF_OK;
}

extern "C" int sf_mc_count(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void* ws, uint64_t ws_bytes,
                           uint32_t* counts2, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mc_check(vol, nx, ny, nz, ws, ws_bytes, "mc_count")) return rc;
  if (!counts2) SF_FAIL(SF_ERR_INVALID, "mc_count: null pointer");
  const McWs w = mc_ws(ws, nx, ny, nz);
  const uint32_t nb = mc_blocks(nx, ny, nz);
  const McDims d{nx, ny, nz};
  k_mc_classify<<<nb, MC_NT, 0, st>>>(vol, d, iso, w.code, w.bsum);
  SF_CHECK_LAUNCH("mc_classify");
  k_mc_scan<<<1, MC_NT, 0, st>>>(w.bsum, nb, w.boff, counts2);
  SF_CHECK_LAUNCH("mc_scan");
  return SF_OK;
}

extern "C" int sf_mc_emit(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void* ws, uint64_t ws_bytes, float* verts,
                          int32_t* faces, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mc_check(vol, nx, ny, nz, ws, ws_bytes, "mc_emit")) return rc;
  const McWs w = mc_ws(ws, nx, ny, nz);
  const uint32_t nb = mc_blocks(nx, ny, nz);
  const McDims d{nx, ny, nz};
  k_mc_emit_verts<<<nb, MC_NT, 0, st>>>(vol, d, iso, w.code, w.boff, verts, w.vbase);
  SF_CHECK_LAUNCH("mc_emit_verts");
  k_mc_emit_faces<<<nb, MC_NT, 0, st>>>(d, w.code, w.boff, w.vbase, faces);
  SF_CHECK_LAUNCH("mc_emit_faces");
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------------------- mesh clean-up
// Connected components and floater removal (mesh_clean.h).
static bool mcl_sizes_ok(uint32_t V, uint32_t F) { return V < (1u << 31) && F < (1u << 31); }

extern "C" uint64_t sf_mesh_components_workspace_bytes(uint32_t V, uint32_t F) {
  if (!mcl_sizes_ok(V, F)) return 0;
  return align256((uint64_t)V * sizeof(uint32_t));      // parent u32 [V]
}

extern "C" int sf_mesh_components(const int32_t* faces, uint32_t F, uint32_t V, int32_t* vertex_label, int32_t* face_label,
                                  uint32_t* faces_per_label, uint32_t* counts3, void* ws, uint64_t ws_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!mcl_sizes_ok(V, F)) SF_FAIL(SF_ERR_INVALID, "mesh_components: need V < 2^31 and F < 2^31");
  if ((F && !faces) || (V && (!vertex_label || !faces_per_label || !ws)) || !counts3)
    SF_FAIL(SF_ERR_INVALID, "mesh_components: null pointer");
  if (ws_bytes < sf_mesh_components_workspace_bytes(V, F)) SF_FAIL(SF_ERR_INVALID, "mesh_components: workspace too small");
  uint32_t* parent = (uint32_t*)ws;
  const uint32_t gv = sf_grid_cap(sf_div_up(V, MCL_NT)), gf = sf_grid_cap(sf_div_up(F, MCL_NT));
  k_cc_init<<<gv, MCL_NT, 0, st>>>(parent, faces_per_label, counts3, V);
  SF_CHECK_LAUNCH("mesh_components init");
  if (F && V) {
    k_cc_hook<<<gf, MCL_NT, 0, st>>>(faces, F, V, parent);
    SF_CHECK_LAUNCH("mesh_components hook");
  }
  if (V) {
    k_cc_flatten<<<gv, MCL_NT, 0, st>>>(parent, V, vertex_label);
    SF_CHECK_LAUNCH("mesh_components flatten");
  }
  if (F) {
    k_cc_count<<<gf, MCL_NT, 0, st>>>(faces, F, V, vertex_label, face_label, faces_per_label, counts3);
    SF_CHECK_LAUNCH("mesh_components count");
  }
  if (F && V) {
    k_cc_stats<<<gv, MCL_NT, 0, st>>>(faces_per_label, V, counts3);
    SF_CHECK_LAUNCH("mesh_components stats");
  }
  return SF_OK;
}

// Workspace: vert_keep u8 [V] | face_keep u8 [F] | remap u32 [V] | bsum u32 [2 * nblk] | boff u32 [2 * nblk]
struct MclWs { uint8_t* vert_keep; uint8_t* face_keep; uint32_t* remap; uint32_t* bsum; uint32_t* boff; };

static uint32_t mcl_blocks(uint32_t V, uint32_t F) {
  const uint32_t n = V > F ? V : F;
  return n ? sf_div_up(n, MC_BLOCK) : 1;
}

static MclWs mcl_ws(void* ws, uint32_t V, uint32_t F) {
  const uint64_t nb = mcl_blocks(V, F);
  char* b = (char*)ws;
  MclWs w;
  w.vert_keep = (uint8_t*)b;
  b += align256(V);
  w.face_keep = (uint8_t*)b;
  b += align256(F);
  w.remap = (uint32_t*)b;
  b += align256((uint64_t)V * 4);
  w.bsum = (uint32_t*)b;
  b += align256(nb * 8);
  w.boff = (uint32_t*)b;
  return w;
}

extern "C" uint64_t sf_mesh_filter_workspace_bytes(uint32_t V, uint32_t F) {
  if (!mcl_sizes_ok(V, F)) return 0;
  return align256(V) + align256(F) + align256((uint64_t)V * 4) + 2 * align256((uint64_t)mcl_blocks(V, F) * 8);
}

static int mcl_filter_check(uint32_t V, uint32_t F, const int32_t* faces, void* ws, uint64_t ws_bytes, const char* what) {
  if (!mcl_sizes_ok(V, F)) SF_FAIL(SF_ERR_INVALID, "%s: need V < 2^31 and F < 2^31", what);
  if ((F && !faces) || !ws) SF_FAIL(SF_ERR_INVALID, "%s: null pointer", what);
  if (ws_bytes < sf_mesh_filter_workspace_bytes(V, F)) SF_FAIL(SF_ERR_INVALID, "%s: workspace too small", what);
  return SF_OK;
}

extern "C" int sf_mesh_filter_count(const int32_t* faces, uint32_t F, uint32_t V, const int32_t* vertex_label,
                                    const uint32_t* faces_per_label, const uint32_t* counts3, uint32_t min_faces, double min_fraction,
                                    void* ws, uint64_t ws_bytes, uint32_t* counts2, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mcl_filter_check(V, F, faces, ws, ws_bytes, "mesh_filter_count")) return rc;
  if ((V && (!vertex_label || !faces_per_label)) || !counts3 || !counts2) SF_FAIL(SF_ERR_INVALID, "mesh_filter_count: null pointer");
  if (!isfinite(min_fraction) || min_fraction < 0.0 || min_fraction > 1.0)
    SF_FAIL(SF_ERR_INVALID, "mesh_filter_count: min_fraction must be finite and in [0, 1]");
  const MclWs w = mcl_ws(ws, V, F);
  const uint32_t nb = mcl_blocks(V, F);
  if (V) {
    k_flt_zero<<<sf_grid_cap(sf_div_up(V, MCL_NT)), MCL_NT, 0, st>>>(w.vert_keep, V);
    SF_CHECK_LAUNCH("mesh_filter zero");
  }
  if (F) {
    k_flt_flags<<<sf_grid_cap(sf_div_up(F, MCL_NT)), MCL_NT, 0, st>>>(faces, F, V, vertex_label, faces_per_label, counts3, min_faces,
                                                                     min_fraction, w.face_keep, w.vert_keep);
    SF_CHECK_LAUNCH("mesh_filter flags");
  }
  k_flt_bsum<<<nb, MC_NT, 0, st>>>(w.vert_keep, V, w.face_keep, F, w.bsum);
  SF_CHECK_LAUNCH("mesh_filter block sums");
  k_mc_scan<<<1, MC_NT, 0, st>>>(w.bsum, nb, w.boff, counts2);
  SF_CHECK_LAUNCH("mesh_filter scan");
  return SF_OK;
}

extern "C" int sf_mesh_filter_emit(const float* verts, const int32_t* faces, uint32_t F, uint32_t V, void* ws, uint64_t ws_bytes,
                                   float* out_verts, int32_t* out_faces, int32_t* vertex_ids, int32_t* face_ids, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mcl_filter_check(V, F, faces, ws, ws_bytes, "mesh_filter_emit")) return rc;
  if (V && !verts) SF_FAIL(SF_ERR_INVALID, "mesh_filter_emit: null pointer");
  const MclWs w = mcl_ws(ws, V, F);
  if (V) {
    k_flt_emit_verts<<<sf_div_up(V, MC_BLOCK), MC_NT, 0, st>>>((const uint32_t*)verts, V, w.vert_keep, w.boff, (uint32_t*)out_verts,
                                                              vertex_ids, w.remap);
    SF_CHECK_LAUNCH("mesh_filter emit vertices");
  }
  if (F) {
    k_flt_emit_faces<<<sf_div_up(F, MC_BLOCK), MC_NT, 0, st>>>(faces, F, w.face_keep, w.boff, w.remap, out_faces, face_ids);
    SF_CHECK_LAUNCH("mesh_filter emit faces");
  }
  return SF_OK;
}

// Mesh clean-up kernels (gfx950): connected components of an indexed triangle mesh by lock-free union-find, per-component face
// counts, and the order-preserving removal of small components (floaters) in the count / emit shape of marching cubes.  Plain C++
// over sf_dev.h, so tests/hostemu compiles the same source for the CPU; the host entry points are in mesh.hip.  DESIGN.md 9.6.
//
// Components.  parent[v] <= v at all times, parent[v] == v marks a root.  init: every vertex its own root.  hook: each valid face
// unites (a, b) and (b, c): find both roots, put the LARGER root under the smaller with one compare-and-swap on the larger root's
// own word, retry from the new roots if it lost.  find halves the path behind it with atomicMin.  flatten: label[v] = root of v.
// Every link points to a smaller index of the same tree, so a tree's root is its smallest vertex: the label of a component is the
// smallest vertex index in it -- a function of the mesh alone, whatever the order in which the atomics retire.  Vertices are
// connected by INDEX only: coincident but unwelded vertices stay apart.  A face with an index outside [0, V) is invalid: it
// connects nothing, gets label -1 and is counted.  A face with a repeated index is valid.
//
// Filter.  A component is kept iff n >= min_faces and n >= ceil(min_fraction * largest) (double); a face iff it is valid and its
// component is kept; a vertex iff a kept face names it.  count: keep flags, per-block sums (MC_BLOCK elements per workgroup) and
// k_mc_scan's exclusive scan of them (one workgroup, any number of blocks) -> {V', F'}.  emit: each block re-scans its flags and
// writes the kept rows in their old order: verts' (bit copies), faces' (indices remapped), vertex_ids, face_ids.
#pragma once
#include "mesh_kernels.h"

#define MCL_NT 256           // threads of the element-wise kernels (grid-stride; the scans use MC_NT / MC_BLOCK of mesh_kernels.h)

SF_DEV bool mcl_face_valid(const int32_t* __restrict__ faces, uint64_t f, uint32_t V, uint32_t* a, uint32_t* b, uint32_t* c) {
  *a = (uint32_t)faces[3 * f];            // a negative index is >= 2^31 as unsigned, and V < 2^31
  *b = (uint32_t)faces[3 * f + 1];
  *c = (uint32_t)faces[3 * f + 2];
  return *a < V && *b < V && *c < V;
}

// parent[v] = v, faces_per_label[v] = 0, counts3 = {0, 0, 0}
SF_KERNEL(MCL_NT) void k_cc_init(uint32_t* __restrict__ parent, uint32_t* __restrict__ faces_per_label, uint32_t* __restrict__ counts3,
                                uint32_t V) {
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
  if (t0 < 3) counts3[t0] = 0;
  for (uint64_t v = t0; v < V; v += stride) {      // terminates: v grows by stride >= 1
    parent[v] = (uint32_t)v;
    faces_per_label[v] = 0;
  }
}

// A root of x's tree at the time it was read, halving the path on the way (parent[x] = grandparent, by atomicMin so that a link only
// ever moves to a smaller index of the same tree).
SF_DEV uint32_t cc_find(uint32_t* parent, uint32_t x) {
  for (;;) {      // terminates: parent[y] < y for a non-root y, so x strictly decreases every trip and is bounded below by 0
    const uint32_t p = sf_atomic_load_u32(parent + x);
    if (p == x) return x;
    const uint32_t g = sf_atomic_load_u32(parent + p);
    if (g < p) (void)sf_atomic_min_u32(parent + x, g);
    x = g;                                          // g <= p < x
  }
}

// Unites the trees of u and v.  Lock-free: the compare-and-swap succeeds only while hi is still a root (then lo < hi lies in another
// tree, whose root is <= lo); it fails only because another lane has hooked hi in the meantime, and no lane waits for another.
SF_DEV void cc_union(uint32_t* parent, uint32_t u, uint32_t v) {
  for (;;) {      // terminates: after a failed trip hi is no root any more, so find returns a smaller root for it: u + v strictly decreases
    u = cc_find(parent, u);
    v = cc_find(parent, v);
    if (u == v) return;
    const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
    if (sf_atomic_cas_u32(parent + hi, hi, lo) == hi) return;
  }
}

SF_KERNEL(MCL_NT) void k_cc_hook(const int32_t* __restrict__ faces, uint32_t F, uint32_t V, uint32_t* parent) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += stride) {      // terminates: f grows by stride >= 1
    uint32_t a, b, c;
    if (!mcl_face_valid(faces, f, V, &a, &b, &c)) continue;
    cc_union(parent, a, b);
    cc_union(parent, b, c);
  }
}

// label[v] = root of v; every hook has retired (kernel boundary), so the roots are final and only the halving still writes
SF_KERNEL(MCL_NT) void k_cc_flatten(uint32_t* parent, uint32_t V, int32_t* __restrict__ label) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride)        // terminates: v grows by stride >= 1
    label[v] = (int32_t)cc_find(parent, (uint32_t)v);
}

// face_label[f] = label of the face's vertices or -1 (face_label may be NULL); faces_per_label[label] += 1; counts3[2] += invalid
SF_KERNEL(MCL_NT) void k_cc_count(const int32_t* __restrict__ faces, uint32_t F, uint32_t V, const int32_t* __restrict__ label,
                                 int32_t* __restrict__ face_label, uint32_t* faces_per_label, uint32_t* counts3) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += stride) {      // terminates: f grows by stride >= 1
    uint32_t a, b, c;
    const bool ok = mcl_face_valid(faces, f, V, &a, &b, &c);
    const int32_t l = ok ? label[a] : -1;
    if (face_label) face_label[f] = l;
    (void)sf_atomic_add_u32(ok ? faces_per_label + l : counts3 + 2, 1u);
  }
}

// counts3[0] = labels with at least one face, counts3[1] = the largest face count (integer add / max: order-independent)
SF_KERNEL(MCL_NT) void k_cc_stats(const uint32_t* __restrict__ faces_per_label, uint32_t V, uint32_t* counts3) {
  SF_SHARED uint32_t acc[2];
  if (threadIdx.x == 0) acc[0] = acc[1] = 0;
  sf_sync();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride) {      // terminates: v grows by stride >= 1
    const uint32_t n = faces_per_label[v];
    if (!n) continue;
    (void)sf_atomic_add_u32(&acc[0], 1u);
    (void)sf_atomic_max_u32(&acc[1], n);
  }
  sf_sync();
  if (threadIdx.x == 0 && acc[0]) {
    (void)sf_atomic_add_u32(counts3, acc[0]);
    (void)sf_atomic_max_u32(counts3 + 1, acc[1]);
  }
}

// ------------------------------------------------------------------------------------------------------------------------ filter
SF_KERNEL(MCL_NT) void k_flt_zero(uint8_t* __restrict__ vert_keep, uint32_t V) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride) vert_keep[v] = 0;      // terminates: v grows
}

// face_keep[f], and vert_keep[v] = 1 for the vertices of a kept face (every writer stores the same 1)
SF_KERNEL(MCL_NT) void k_flt_flags(const int32_t* __restrict__ faces, uint32_t F, uint32_t V, const int32_t* __restrict__ label,
                                  const uint32_t* __restrict__ faces_per_label, const uint32_t* __restrict__ counts3, uint32_t min_faces,
                                  double min_fraction, uint8_t* __restrict__ face_keep, uint8_t* vert_keep) {
  const double need = ceil(min_fraction * (double)counts3[1]);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += stride) {      // terminates: f grows by stride >= 1
    uint32_t a, b, c;
    bool keep = mcl_face_valid(faces, f, V, &a, &b, &c);
    if (keep) {
      const uint32_t l = (uint32_t)label[a];
      const uint32_t n = l < V ? faces_per_label[l] : 0u;      // a label that is no vertex index (not sf_mesh_components' output) keeps nothing
      keep = n > 0 && n >= min_faces && (double)n >= need;
    }
    face_keep[f] = keep ? 1 : 0;
    if (keep) vert_keep[a] = vert_keep[b] = vert_keep[c] = 1;
  }
}

SF_DEV uint32_t mcl_flags4(const uint8_t* __restrict__ keep, uint32_t n, uint64_t i0, uint32_t* m) {
  uint32_t s = 0;
  for (uint32_t u = 0; u < MC_ITEMS; ++u) s += (m[u] = i0 + u < n ? keep[i0 + u] : 0u);
  return s;
}

// bsum[2 b] / bsum[2 b + 1] = kept vertices / faces among elements [b * MC_BLOCK, (b + 1) * MC_BLOCK): the input of k_mc_scan
SF_KERNEL(MC_NT) void k_flt_bsum(const uint8_t* __restrict__ vert_keep, uint32_t V, const uint8_t* __restrict__ face_keep, uint32_t F,
                                uint32_t* __restrict__ bsum) {
  const uint64_t i0 = (uint64_t)blockIdx.x * MC_BLOCK + (uint64_t)threadIdx.x * MC_ITEMS;
  uint32_t m[MC_ITEMS], tv, tf;
  const uint32_t nv = mcl_flags4(vert_keep, V, i0, m), nf = mcl_flags4(face_keep, F, i0, m);
  mc_block_scan(nv, &tv);
  mc_block_scan(nf, &tf);
  if (threadIdx.x == 0) {
    bsum[2 * blockIdx.x] = tv;
    bsum[2 * blockIdx.x + 1] = tf;
  }
}

// kept vertices in their old order: three words per row copied as bits, the old index, and remap[old] = new for the faces
SF_KERNEL(MC_NT) void k_flt_emit_verts(const uint32_t* __restrict__ verts, uint32_t V, const uint8_t* __restrict__ vert_keep,
                                      const uint32_t* __restrict__ boff, uint32_t* __restrict__ out_verts, int32_t* __restrict__ vertex_ids,
                                      uint32_t* __restrict__ remap) {
  const uint64_t i0 = (uint64_t)blockIdx.x * MC_BLOCK + (uint64_t)threadIdx.x * MC_ITEMS;
  uint32_t m[MC_ITEMS], tot;
  const uint32_t n = mcl_flags4(vert_keep, V, i0, m);
  uint64_t id = boff[2 * blockIdx.x] + mc_block_scan(n, &tot);
  for (uint32_t u = 0; u < MC_ITEMS; ++u) {
    if (!m[u]) continue;
    const uint64_t v = i0 + u;
    out_verts[3 * id] = verts[3 * v];
    out_verts[3 * id + 1] = verts[3 * v + 1];
    out_verts[3 * id + 2] = verts[3 * v + 2];
    vertex_ids[id] = (int32_t)v;
    remap[v] = (uint32_t)id;
    ++id;
  }
}

// kept faces in their old order with their indices remapped, and the old index
SF_KERNEL(MC_NT) void k_flt_emit_faces(const int32_t* __restrict__ faces, uint32_t F, const uint8_t* __restrict__ face_keep,
                                      const uint32_t* __restrict__ boff, const uint32_t* __restrict__ remap, int32_t* __restrict__ out_faces,
                                      int32_t* __restrict__ face_ids) {
  const uint64_t i0 = (uint64_t)blockIdx.x * MC_BLOCK + (uint64_t)threadIdx.x * MC_ITEMS;
  uint32_t m[MC_ITEMS], tot;
  const uint32_t n = mcl_flags4(face_keep, F, i0, m);
  uint64_t id = boff[2 * blockIdx.x + 1] + mc_block_scan(n, &tot);
  for (uint32_t u = 0; u < MC_ITEMS; ++u) {
    if (!m[u]) continue;
    const uint64_t f = i0 + u;
    out_faces[3 * id] = (int32_t)remap[faces[3 * f]];
    out_faces[3 * id + 1] = (int32_t)remap[faces[3 * f + 1]];
    out_faces[3 * id + 2] = (int32_t)remap[faces[3 * f + 2]];
    face_ids[id] = (int32_t)f;
    ++id;
  }
}

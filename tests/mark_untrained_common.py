"""Shared pieces of the mark_untrained_grid tests (sf_occ_mark_untrained; sparsefusion_amd/csrc/occ_mark.h): (a) a vectorised torch
float32 restatement of the kernel's arithmetic, operation for operation; (b) a float64 restatement of the reference's formula
(external/nerf/renderer.py:411-433) with the margin of every camera-cell pair; (c) the ring-of-cameras scenes; the checksum of the
golden; the ctypes harness of tests/hostemu/occ_mark_emu.cpp.

THE RULE (restated from occ_mark.h), float32, one rounding per operation, in this order:
    w_a = 2 * float(c_a) / float(H - 1) - 1;  bound_c = min(2^cas, bound);  hg = bound_c / H;  s = bound_c - hg;  hg2 = hg * 2
    p_a = w_a * s;  q_a = p_a - t_a;  cam_j = (q_0 R_0j + q_1 R_1j) + q_2 R_2j;  rx = cx / fx, ry = cy / fy (float32 division)
    covered = cam_2 > 0 and |cam_0| < rx * cam_2 + hg2 and |cam_1| < ry * cam_2 + hg2
Cells are in storage (Morton) order: index i holds cell (x, y, z) = (compact(i), compact(i >> 1), compact(i >> 2))."""
import ctypes as C
import math
import os
import subprocess

import torch

MARGIN = 1e-5                  # coordinates are below 8: one ulp is 9.5e-7; a three-term dot product and a multiply-add accumulate ~6 ulp
EXCLUDED_MAX = 2e-4            # at most 0.02 % of all pairs may lie below MARGIN (a condition on the scenes, not a tolerance)
SCENES = dict(A=dict(B=3, r=1.8, bound=2.0, intrinsic=(400.0, 400.0, 100.0, 100.0)),
              B=dict(B=5, r=3.0, bound=4.0, intrinsic=(300.0, 320.0, 64.0, 48.0)),
              C=dict(B=70, r=1.5, bound=1.0, intrinsic=(500.0, 500.0, 64.0, 64.0)))


def cascades(bound):
    return 1 + math.ceil(math.log2(bound))


def ring_cameras(B, r):
    """[B, 4, 4] float32 camera-to-world poses on a ring, looking at the origin: centre r (cos th cos ph, sin ph, sin th cos ph) with
    th = 2 pi i / B + 0.3, ph = 0.4 sin(1.7 i), plus 0.05 randn(3) from Generator().manual_seed(B); columns x = normalize(cross((0, 1,
    0), z)), y = cross(z, x), z = -c / |c|; computed in float64 and rounded to float32."""
    g = torch.Generator().manual_seed(B)
    jitter = 0.05 * torch.randn(B, 3, generator=g, dtype=torch.float64)
    i = torch.arange(B, dtype=torch.float64)
    th, ph = 2 * math.pi * i / max(B, 1) + 0.3, 0.4 * torch.sin(1.7 * i)
    c = r * torch.stack([torch.cos(th) * torch.cos(ph), torch.sin(ph), torch.sin(th) * torch.cos(ph)], -1) + jitter
    z = -c / c.norm(dim=-1, keepdim=True)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).expand(B, 3)
    x = torch.linalg.cross(up, z)
    x = x / x.norm(dim=-1, keepdim=True)
    y = torch.linalg.cross(z, x)
    poses = torch.zeros(B, 4, 4, dtype=torch.float64)
    poses[:, :3, 0], poses[:, :3, 1], poses[:, :3, 2], poses[:, :3, 3], poses[:, 3, 3] = x, y, z, c, 1.0
    return poses.float()


def scene(name):
    s = SCENES[name]
    return dict(poses=ring_cameras(s["B"], s["r"]), intrinsics=torch.tensor(s["intrinsic"], dtype=torch.float32).repeat(s["B"], 1),
                bound=s["bound"], C=cascades(s["bound"]))


def compact_bits(x):
    x = x & 0x49249249
    x = (x | (x >> 2)) & 0xc30c30c3
    x = (x | (x >> 4)) & 0x0f00f00f
    x = (x | (x >> 8)) & 0xff0000ff
    x = (x | (x >> 16)) & 0x0000ffff
    return x


def cells(H):
    """[H^3, 3] int64 cell coordinates in storage order"""
    i = torch.arange(H ** 3, dtype=torch.int64)
    return torch.stack([compact_bits(i), compact_bits(i >> 1), compact_bits(i >> 2)], -1)


# ------------------------------------------------------------------------------------------------------------ (a) the kernel, float32
def unit_coords_a(H, device="cpu"):
    """w [3, H^3] float32, formed on the CPU (IEEE division of two tensors) whatever the device of the rest"""
    c = cells(H).t().contiguous().float()
    w = (2.0 * c) / torch.full_like(c, float(H - 1)) - 1.0
    return w.to(device)


def cascade_consts_a(bound, cas, H):
    f = lambda v: torch.tensor(v, dtype=torch.float32)                        # noqa: E731
    bc = torch.minimum(f(2.0 ** cas), f(bound))
    hg = bc / f(float(H))
    return bc - hg, hg * f(2.0)                                               # s, hg2 (0-dim float32 tensors)


def ratios_a(intrinsics):
    K = intrinsics.float().cpu()
    return K[:, 2] / K[:, 0], K[:, 3] / K[:, 1]                               # float32 tensor / tensor on the CPU: IEEE division


def covered_a(p, pose, rx, ry, hg2):
    """one camera against the points p [3, N] of one cascade -> bool [N]; pose [4, 4], rx / ry / hg2 0-dim, all float32 on p's device"""
    q0, q1, q2 = p[0] - pose[0, 3], p[1] - pose[1, 3], p[2] - pose[2, 3]
    cx = (q0 * pose[0, 0] + q1 * pose[1, 0]) + q2 * pose[2, 0]
    cy = (q0 * pose[0, 1] + q1 * pose[1, 1]) + q2 * pose[2, 1]
    cz = (q0 * pose[0, 2] + q1 * pose[1, 2]) + q2 * pose[2, 2]
    return (cz > 0) & (cx.abs() < rx * cz + hg2) & (cy.abs() < ry * cz + hg2)


def count_a(poses, intrinsics, bound, C_, H, device="cpu", zero_hg=False):
    """count [C, H^3] int32 of restatement (a) on `device` (elementwise torch float32 ops: one rounding each, never contracted).
    zero_hg: the test without the cell allowance (hg2 = 0), for the poses_from_cameras check."""
    w = unit_coords_a(H, device)
    P = poses.float().to(device)
    rx, ry = (t.to(device) for t in ratios_a(intrinsics))
    out = torch.zeros(C_, H ** 3, dtype=torch.int32, device=device)
    for cas in range(C_):
        s, hg2 = cascade_consts_a(bound, cas, H)
        p = w * s.to(device)
        hg2 = torch.zeros((), device=device) if zero_hg else hg2.to(device)
        for b in range(P.shape[0]):
            out[cas] += covered_a(p, P[b], rx[b], ry[b], hg2)
    return out


def apply_a(grid, count):
    """the grid after marking and the number of cells marked"""
    g = grid.clone()
    g[count == 0] = -1.0
    return g, int((count == 0).sum())


# ------------------------------------------------------------------------------------------------- (b) the reference formula, float64
def covered_b(H, pose, intrinsic, bound, cas, w64=None):
    """one camera, one cascade, float64 -> (covered bool [H^3], margin float64 [H^3] = min(|cam_z|, |rhs_x - |cam_x||, |rhs_y - |cam_y||))"""
    if w64 is None:
        w64 = unit_coords_b(H)
    bc = min(2.0 ** cas, float(bound))
    hg = bc / H
    P = pose.double()
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    cam = (w64 * (bc - hg) - P[:3, 3]) @ P[:3, :3]                            # [H^3, 3]
    rhs_x, rhs_y = cx / fx * cam[:, 2] + hg * 2, cy / fy * cam[:, 2] + hg * 2
    cov = (cam[:, 2] > 0) & (cam[:, 0].abs() < rhs_x) & (cam[:, 1].abs() < rhs_y)
    margin = torch.minimum(cam[:, 2].abs(), torch.minimum((rhs_x - cam[:, 0].abs()).abs(), (rhs_y - cam[:, 1].abs()).abs()))
    return cov, margin


def unit_coords_b(H):
    return 2.0 * cells(H).double() / (H - 1) - 1.0                            # [H^3, 3]


def compare_a_b(sc, H):
    """(a) against (b) pair by pair -> dict(pairs, excluded, disagree_kept, ambiguous [C, H^3] bool, count_a [C, H^3] int32):
    `excluded` pairs have a float64 margin below MARGIN; `disagree_kept` counts the others on which (a) and (b) differ; a cell is
    `ambiguous` when it holds an excluded pair and no kept pair covers it -- its marked state may depend on the rounding."""
    w32, w64 = unit_coords_a(H), unit_coords_b(H)
    rx, ry = ratios_a(sc["intrinsics"])
    B, C_ = sc["poses"].shape[0], sc["C"]
    cnt = torch.zeros(C_, H ** 3, dtype=torch.int32)
    has_excl = torch.zeros(C_, H ** 3, dtype=torch.bool)
    kept_cov = torch.zeros(C_, H ** 3, dtype=torch.bool)
    excluded = disagree = 0
    for cas in range(C_):
        s, hg2 = cascade_consts_a(sc["bound"], cas, H)
        p = w32 * s
        for b in range(B):
            a = covered_a(p, sc["poses"][b], rx[b], ry[b], hg2)
            cov, margin = covered_b(H, sc["poses"][b], sc["intrinsics"][b], sc["bound"], cas, w64)
            keep = margin >= MARGIN
            excluded += int((~keep).sum())
            disagree += int(((a != cov) & keep).sum())
            cnt[cas] += a
            has_excl[cas] |= ~keep
            kept_cov[cas] |= cov & keep
    return dict(pairs=C_ * B * H ** 3, excluded=excluded, disagree_kept=disagree, ambiguous=has_excl & ~kept_cov, count_a=cnt)


# -------------------------------------------------------------------------------------------------------------------------- golden
GOLDEN_SCENE, GOLDEN_H, GOLDEN_ROWS, GOLDEN_ROW_SEED = "B", 128, 4096, 11


def mask_checksum(mask):
    """tests/golden/make_golden_occ.py's bitfield_checksum, of a bool tensor"""
    m = mask.reshape(-1)
    w = (torch.arange(m.numel()) % 251 + 1).long()
    return int((m.long() * w).sum())


def golden_rows(numel):
    return torch.randperm(numel, generator=torch.Generator().manual_seed(GOLDEN_ROW_SEED))[:GOLDEN_ROWS].clone()


def check_against_golden(G, count, n_marked, ambiguous=None):
    """count [C, H^3] (CPU, any integer dtype) and the returned n_marked against the golden of the reference's own function: equal
    totals, per-cascade counts, checksum and sampled rows.  Only if they are not all equal, `ambiguous` (compare_a_b) names the cells
    where a difference from the reference's float32 matmul is allowed -- there and nowhere else -- and the outcome is printed.
    Returns True when everything was equal."""
    marked = count == 0
    per = [int(m.sum()) for m in marked]
    rows_equal = torch.equal(count.reshape(-1)[G["rows"]].long(), G["row_counts"].long())
    assert n_marked == sum(per)
    if n_marked == G["n_marked"] and per == G["per_cascade"] and mask_checksum(marked) == G["checksum"] and rows_equal:
        return True
    assert ambiguous is not None and int(ambiguous.sum()) > 0, (n_marked, per, G["n_marked"], G["per_cascade"], rows_equal)
    amb_per = [int(a.sum()) for a in ambiguous]
    print(f"marked per cascade {per} vs the reference's {G['per_cascade']}: allowed to differ on the {amb_per} cells that hold an excluded pair")
    assert all(abs(p - g) <= a for p, g, a in zip(per, G["per_cascade"], amb_per)), \
        f"marked per cascade {per} vs reference {G['per_cascade']}: more than the {amb_per} cells that hold an excluded pair"
    sure = ~ambiguous.reshape(-1)[G["rows"]]
    assert torch.equal(count.reshape(-1)[G["rows"]].long()[sure], G["row_counts"].long()[sure]), \
        "sampled counts differ outside the cells that hold an excluded pair"
    return False


# ------------------------------------------------------------------------------------- small shapes (emulation and GPU entry tests)
# (H, C, B): every H with every C and B somewhere; the 70-camera loop at H = 32 once per mode
SHAPES = [(4, 1, 0), (4, 2, 1), (4, 3, 3), (4, 3, 70), (8, 1, 3), (8, 2, 70), (8, 2, 130), (8, 3, 0), (8, 3, 1), (32, 1, 1), (32, 2, 3), (32, 3, 70)]
SHAPE_BOUND = {1: 1.0, 2: 2.0, 3: 4.0}
SHAPE_RADIUS = {1: 1.5, 2: 1.8, 3: 3.0}


def shape_cameras(B, C_):
    K = torch.tensor([300.0, 320.0, 64.0, 48.0]).repeat(B, 1)
    if B > 1:
        K[1] = torch.tensor([400.0, 380.0, 100.0, 90.0])                      # per-camera intrinsics
    return ring_cameras(B, SHAPE_RADIUS[C_]), K


# ------------------------------------------------------------------------------------------------------------------ host emulation
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_SO = os.path.join(_HERE, "_build", "libocc_mark_emu.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_handle = None


def emu_available():
    return os.path.exists(CLANG)


def _emu():
    global _handle
    if _handle is None:
        csrc = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
        deps = [os.path.join(_HERE, f) for f in ("occ_mark_emu.cpp", "hip_emu.h")] + \
               [os.path.join(csrc, f) for f in ("occ_mark.h", "ngp_device.h", "sf_dev.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call([CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + _HERE, "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-Wno-source-uses-openmp", "-ffp-contract=off", deps[0], "-o", _SO,
                                   "-lpthread"])
        _handle = C.CDLL(_SO)
        _handle.emu_occ_mark_untrained.restype = None
    return _handle


def emu_mark(poses, intrinsics, bound, grid, with_count, max_blocks=0):
    """k_occ_mark_untrained on CPU fibers -> (grid after, count [C, H^3] int32 pre-filled with -7 or None, n_marked); max_blocks > 0
    caps the grid, so that the workgroups stride over the tiles as they do at 128^3"""
    g = grid.clone().contiguous()
    C_, H3 = g.shape
    H = round(H3 ** (1 / 3))
    P, K = poses.float().contiguous(), intrinsics.float().contiguous()
    count = torch.full((C_, H3), -7, dtype=torch.int32) if with_count else None
    n = torch.full((1,), -1, dtype=torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)      # noqa: E731
    _emu().emu_occ_mark_untrained(p(P), p(K), C.c_uint32(P.shape[0]), C.c_float(bound), C.c_uint32(C_), C.c_uint32(H), p(g), p(count),
                                  p(n), C.c_uint32(max_blocks))
    return g, count, int(n)


def prefilled_grid(C_, H, seed=5):
    """a mix of 0, positive values and -1"""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(C_, H ** 3, generator=g) * 20
    kind = torch.randint(0, 3, (C_, H ** 3), generator=g)
    return torch.where(kind == 0, torch.zeros_like(v), torch.where(kind == 1, v, -torch.ones_like(v)))

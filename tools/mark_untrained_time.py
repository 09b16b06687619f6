"""Time mark_untrained_grid's launch (sf_occ_mark_untrained, csrc/occ_mark.h) at the project's grid (bound 4: 3 cascades of 128^3
cells) for B = 6 and B = 100 ring cameras, with `count` (all B cameras per cell) and without (a wave stops once all its cells are
covered), next to a torch restatement of the reference's blocked algorithm (external/nerf/renderer.py:394-440: blocks of S^3 cells, chunks of
S cameras, batched matmul, scatter through this library's raymarching.morton3D) on the same GPU.
usage: mark_untrained_time.py [--repeats 30] [--batch 20] [--passes 2] [--loop-repeats 5]
The launch is timed with device events around `--batch` back-to-back calls of the C entry on preallocated buffers (a marked grid is
marked again: the same reads, tests and stores), after a warm-up; per variant the median and the minimum over --repeats batches, the
variants alternating over --passes passes (one line per pass: their difference is the spread).  The loop is timed per call, with a
synchronise, median of --loop-repeats.  Also printed: the cells marked, and whether the loop marks the same cells."""
import argparse, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sparsefusion_amd import raymarching
from sparsefusion_amd.raymarching import backend

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--batch", type=int, default=20)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--loop-repeats", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "mark_untrained_time.py measures on the GPU"
dev = "cuda:0"
BOUND, H = 4.0, 128
CAS = 1 + math.ceil(math.log2(BOUND))
INTR = (300.0, 320.0, 64.0, 48.0)


def ring(B, r=3.0):
    """cameras on a ring of radius r looking at the origin (the scenes of tests/mark_untrained_common.py, without the jitter)"""
    i = torch.arange(B, dtype=torch.float64)
    th, ph = 2 * math.pi * i / B + 0.3, 0.4 * torch.sin(1.7 * i)
    c = r * torch.stack([torch.cos(th) * torch.cos(ph), torch.sin(ph), torch.sin(th) * torch.cos(ph)], -1)
    z = -c / c.norm(dim=-1, keepdim=True)
    x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).expand(B, 3), z)
    x = x / x.norm(dim=-1, keepdim=True)
    y = torch.linalg.cross(z, x)
    P = torch.zeros(B, 4, 4, dtype=torch.float64)
    P[:, :3, 0], P[:, :3, 1], P[:, :3, 2], P[:, :3, 3], P[:, 3, 3] = x, y, z, c, 1.0
    return P.float().to(dev)


def blocked_loop(poses, S=64):
    """The blocked algorithm the reference uses, restated: the grid in blocks of S^3 cells, the cameras in chunks of S, the camera
    coordinates of a whole (chunk, block) by one batched matmul, the per-cell sums scattered through morton3D -> [C, H^3] float32."""
    fx, fy, cx, cy = INTR
    tan_x, tan_y = cx / fx, cy / fy
    R, t = poses[:, :3, :3], poses[:, :3, 3]
    count = torch.zeros(CAS, H ** 3, device=dev)
    axis = torch.arange(H, dtype=torch.int32, device=dev)
    for x0 in range(0, H, S):
        for y0 in range(0, H, S):
            for z0 in range(0, H, S):
                cell = torch.stack(torch.meshgrid(axis[x0:x0 + S], axis[y0:y0 + S], axis[z0:z0 + S], indexing='ij'), -1).reshape(-1, 3)
                slot = raymarching.morton3D(cell).long()
                unit = 2 * cell.float() / (H - 1) - 1                                   # [n, 3] in [-1, 1]
                for cas in range(CAS):
                    extent = min(2 ** cas, BOUND)
                    half = extent / H
                    centre = unit * (extent - half)
                    for b0 in range(0, poses.shape[0], S):
                        cam = (centre[None] - t[b0:b0 + S, None]) @ R[b0:b0 + S]        # [s, n, 3]
                        depth = cam[..., 2]
                        seen = (depth > 0) & (cam[..., 0].abs() < tan_x * depth + 2 * half) & (cam[..., 1].abs() < tan_y * depth + 2 * half)
                        count[cas, slot] += seen.sum(0)
    return count


def timed_launch(poses, intr, grid, count, n_marked):
    def call():
        backend.occ_mark_untrained(poses, intr, poses.shape[0], BOUND, CAS, H, grid, count, n_marked)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.batch):
            call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / args.batch)                  # us per call
    return statistics.median(ts), min(ts)


def timed_loop(poses):
    blocked_loop(poses)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.loop_repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        c = blocked_loop(poses)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), c


print(f"mark_untrained_grid: {CAS} cascades of {H}^3 cells (bound {BOUND:g}), {CAS * H ** 3 * 4 / 1e6:.1f} MB of grid; launch times in us per call "
      f"(device events around {args.batch} calls, median of {args.repeats} (min)); loop times in ms (median of {args.loop_repeats} (min))")
for B in (6, 100):
    poses = ring(B)
    intr = torch.tensor(INTR, device=dev).repeat(B, 1).contiguous()
    grid = torch.zeros(CAS, H ** 3, device=dev)
    count = torch.empty(CAS, H ** 3, dtype=torch.int32, device=dev)
    n_marked = torch.zeros(1, dtype=torch.int32, device=dev)
    for k in range(args.passes):
        a, a_min = timed_launch(poses, intr, grid, count, n_marked)
        n_count = int(n_marked.item())
        b, b_min = timed_launch(poses, intr, grid, None, n_marked)
        assert int(n_marked.item()) == n_count
        print(f"B = {B:3d}, pass {k}: with count {a:8.1f} ({a_min:.1f}) us, early exit {b:8.1f} ({b_min:.1f}) us, early / count = {b / a:.2f}; "
              f"marked {n_count} of {CAS * H ** 3} ({n_count / (CAS * H ** 3):.1%})")
    c, c_min, ref_count = timed_loop(poses)
    differ = int(((ref_count == 0) != (count == 0)).sum())
    print(f"B = {B:3d}: reference-style blocked loop in torch {c:8.1f} ({c_min:.1f}) ms = {c * 1e3 / a:.0f} x the counting launch; "
          f"cells whose marked state differs from the launch's: {differ}")

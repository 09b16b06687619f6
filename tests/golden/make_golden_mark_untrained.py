"""Golden of the camera-coverage culling from the REAL reference's NeRFRenderer.mark_untrained_grid (external/nerf/renderer.py:379-442;
dev container only).  The function runs unbound on the reference's own cuda_ray network on the CPU; only raymarching.morton3D
underneath is the C oracle (oracle/ref_loader.py stubs).  Scene B of tests/mark_untrained_common.py at H = 128, bound = 4.  The file
holds the configuration, the cameras, the marked totals, 4096 sampled (index, count) rows and a checksum of count == 0 -- not the
25 MB grid."""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_loader  # noqa: E402
import mark_untrained_common as mc  # noqa: E402


def main():
    ref_loader.install()
    if "trimesh" not in sys.modules:                                          # external/nerf/renderer.py imports it at the top
        sys.modules["trimesh"] = types.ModuleType("trimesh")
    from external.nerf import renderer as ref_renderer
    name = mc.GOLDEN_SCENE
    sc = mc.scene(name)
    opt = ref_loader.ngp_opt()
    opt.cuda_ray = True
    opt.bound = int(sc["bound"])
    net = ref_loader.reference_ngp(opt)
    assert net.grid_size == mc.GOLDEN_H and net.cascade == sc["C"]
    net.density_grid.fill_(0.5)
    intrinsic = [float(v) for v in sc["intrinsics"][0]]
    # the reference keeps its per-cell camera count in a local made by torch.zeros_like(self.density_grid): that tensor is kept here
    real_zeros_like, kept = torch.zeros_like, {}

    def zeros_like(t, **kw):
        z = real_zeros_like(t, **kw)
        if t is net.density_grid:
            kept["count"] = z
        return z

    torch.zeros_like = zeros_like
    try:
        ref_renderer.NeRFRenderer.mark_untrained_grid(net, sc["poses"].clone(), intrinsic)
    finally:
        torch.zeros_like = real_zeros_like
    count = kept["count"].round().int()
    marked = net.density_grid == -1
    assert torch.equal(marked, count == 0) and bool((net.density_grid[~marked] == 0.5).all())
    rows = mc.golden_rows(count.numel())
    out = dict(cfg=dict(scene=name, H=mc.GOLDEN_H, **{k: v for k, v in mc.SCENES[name].items()}), poses=sc["poses"],
               intrinsics=sc["intrinsics"], n_marked=int(marked.sum()), per_cascade=[int(m.sum()) for m in marked], rows=rows,
               row_counts=count.reshape(-1)[rows].clone(), checksum=mc.mask_checksum(marked))
    torch.save(out, os.path.join(HERE, "ngp_mark_untrained.pt"))
    print({k: v for k, v in out.items() if not torch.is_tensor(v)},
          f"marked {out['n_marked'] / marked.numel():.1%}, sampled counts 0..{int(out['row_counts'].max())}")


if __name__ == "__main__":
    main()

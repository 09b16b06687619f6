"""Generate tests/golden/ngp_render_shaded.pt: the REAL reference's NeRFNetwork.render (renderer_df.py:643 -> run :310) with
shading='lambertian' on the CPU (oracle/ref_loader.py; development container only), on the teacher field and the 256 rays of
ngp_render.pt, with a given light, ambient_ratio 0.1 and bg_color 1.  Two cases:
  eval    eval mode, perturb=False (deterministic fine samples)
  train   train mode under no_grad, perturb=True; the reference's two draws (rand(N, T) stratified jitter, rand(N, T) inverse-CDF
          draw -- no randn(3): the light is given) are reproduced from `noise_seed` on the CPU generator
The file holds the seeds, the light and the reference's outputs; parameters and rays are re-derived from the seeds by the tests.

    python tests/golden/make_golden_shaded.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from oracle import ngp_ref, ref_loader  # noqa: E402

LIGHT = (0.3, -0.5, 0.81)
RATIO = 0.1
BG = 1
IMAGE_BOUND_CAP = 1e-2          # tests/test_gpu_shaded_render.py: the derived per-ray image bound must stay below this


def rays(view, unit):
    o, d = ngp_ref.circle_rays(16, view=view, unit_dir=unit)
    o[5] = torch.tensor([20.0, 20.0, 20.0]); d[5] = torch.tensor([1.0, 0.0, 0.0])     # a ray that misses the box (as ngp_render.pt)
    return o, d


def draws(noise_seed, N, T=64):
    torch.manual_seed(noise_seed)
    return torch.rand(N, T), torch.rand(N, T)


def main():
    import shaded_common as sc
    base = torch.load(os.path.join(HERE, "ngp_render.pt"))["teacher"]
    cfg = dict(base["cfg"])
    p = ngp_ref.init_params(bound=4, seed=cfg["seed"], table_std=cfg["table_std"], sigma_bias=cfg["sigma_bias"])
    o, d = rays(cfg["view"], cfg["unit_dir"])
    assert torch.equal(o, base["rays_o"]) and torch.equal(d, base["rays_d"])
    light = torch.tensor(LIGHT, dtype=torch.float32)
    light = light / light.norm()
    opt = ref_loader.ngp_opt()
    net = ref_loader.reference_ngp()
    net.load_state_dict({k: p[k] for k in net.state_dict().keys()})
    out = dict(cfg=cfg, light_d=light, ambient_ratio=RATIO, bg_color=BG, epsilon=1e-2)
    noise_seed = 2000 + cfg["seed"]
    for case in ("eval", "train"):
        net.train(case == "train")
        if case == "train":
            uc, uf = draws(noise_seed, o.shape[0])
            torch.manual_seed(noise_seed)                 # the reference draws the same two tensors in this order
        else:
            uc = uf = None
        with torch.no_grad():
            r = net.render(o[None], d[None], staged=False, perturb=case == "train", bg_color=BG, ambient_ratio=RATIO,
                           shading='lambertian', light_d=light, force_all_rays=True, **vars(opt))
        out[case] = dict(noise_seed=noise_seed if case == "train" else None, image=r['image'][0].clone(),
                         depth=r['depth'][0].clone(), weights_sum=r['weights_sum'].clone(), loss_orient=r['loss_orient'].clone())
        # the restatement the tests compare with, and the cap on the GPU test's derived bound
        rs = sc.restated(p, o, d, light, RATIO, BG, uc, uf, training=case == "train")
        err = float((rs["image"] - out[case]["image"]).abs().max())
        rel = abs(float(rs["loss_orient"]) - float(out[case]["loss_orient"])) / float(out[case]["loss_orient"])
        bound = sc.image_bound(rs, RATIO)
        contrast = float((rs["image"] - rs["image_albedo"]).abs().mean())
        print(f"{case}: restatement vs reference image {err:.2e}, loss_orient rel {rel:.2e} ({float(out[case]['loss_orient']):.6e}); "
              f"image bound median {float(np.median(bound)):.2e} max {float(bound.max()):.2e}; shaded - albedo mean {contrast:.3f}")
        assert err <= 1e-6 and rel <= 1e-6
        assert float(bound.max()) <= IMAGE_BOUND_CAP
    torch.save(out, os.path.join(HERE, "ngp_render_shaded.pt"))
    print("wrote ngp_render_shaded.pt", os.path.getsize(os.path.join(HERE, "ngp_render_shaded.pt")), "bytes")


if __name__ == "__main__":
    main()

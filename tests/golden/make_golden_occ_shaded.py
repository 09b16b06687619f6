"""Generate tests/golden/ngp_occ_render_shaded.pt: the REAL reference's occupancy-grid evaluation render (`cuda_ray=True`,
net.eval(); net.render -> run_cuda, external/nerf/renderer_df.py:471-584) on the CPU (oracle/ref_loader.py; development container
only), once with shading='lambertian' and once with shading='albedo', with a given light, ambient_ratio 0.1 and bg_color 1.

The field is ngp_ref.init_params(bound=4, seed=1, table_std=3.0, sigma_bias=1.0); the density bitfield is the ANALYTIC ball of
tests/occ_common.py, copied into the reference's buffer (density_bitfield.copy_) and loaded into the library the same way: it does
not come from update_extra_state, so no cell sits on a threshold and every ray can be held to a bound.  The rays are
occ_common.camera_rays(16).  The file holds the cfg, the light and the reference's outputs; parameters, bitfield and rays are
re-derived by the tests (tests/occ_shaded_common.py).

    python tests/golden/make_golden_occ_shaded.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from oracle import ref_loader  # noqa: E402


def main():
    import occ_shaded_common as oc
    cfg = dict(oc.CFG)
    p = oc.params()
    sc = oc.golden_scene()
    light = oc.unit(oc.LIGHT)
    opt = ref_loader.ngp_opt()
    opt.cuda_ray = True
    net = ref_loader.reference_ngp(opt)
    sd = net.state_dict()
    sd.update({k: p[k] for k in p if k in sd})
    net.load_state_dict(sd)
    net.eval()
    net.density_bitfield.copy_(sc["bits"])
    kw = vars(opt)
    assert kw["max_steps"] == cfg["max_steps"] and kw["dt_gamma"] == cfg["dt_gamma"]
    out = dict(cfg=cfg, light_d=light, ambient_ratio=oc.RATIO, bg_color=oc.BG, epsilon=oc.EPS)
    with torch.no_grad():
        for name, shading in (("shaded", "lambertian"), ("albedo", "albedo")):
            r = net.render(sc["o"][None], sc["d"][None], staged=False, perturb=False, bg_color=oc.BG, ambient_ratio=oc.RATIO,
                           shading=shading, light_d=light, **kw)
            out[name] = dict(image=r['image'][0].clone(), depth=r['depth'][0].clone(), weights_sum=r['weights_sum'][0].clone())
    # the restatement the tests compare with, and the cap on the GPU test's derived bound
    rs = oc.restated(p, sc, light, oc.RATIO, cfg["T_thresh"])
    img, dep = oc.finish(sc, rs["image"], rs["depth"], rs["weights_sum"])
    img_a, _ = oc.finish(sc, rs["image_albedo"], rs["depth_albedo"], rs["weights_sum_albedo"])
    hit = sc["nears"] < sc["fars"]
    e_img = float((img - out["shaded"]["image"]).abs().max())
    e_alb = float((img_a - out["albedo"]["image"]).abs().max())
    e_ws = float((rs["weights_sum"] - out["shaded"]["weights_sum"]).abs().max())
    e_dep = float((dep[hit] - out["shaded"]["depth"][hit]).abs().max())
    bound = oc.image_bound(rs)
    ended = int(((rs["n_samples"] < rs["count"]) & (rs["count"] > 0)).sum())
    contrast = float((out["shaded"]["image"] - out["albedo"]["image"]).abs().mean())
    print(f"restatement vs reference: image {e_img:.2e}, albedo image {e_alb:.2e}, weights_sum {e_ws:.2e}, depth {e_dep:.2e}")
    print(f"rays that hit the ball {int((rs['count'] > 0).sum())}, mean weights_sum {float(out['shaded']['weights_sum'].mean()):.5f}, "
          f"ended by T_thresh {ended}, most samples {int(rs['count'].max())} of {cfg['max_steps']}, shaded - albedo mean {contrast:.3f}")
    print(f"image bound median {float(np.median(bound[rs['count'].numpy() > 0])):.2e} max {float(bound.max()):.2e}")
    assert e_img <= 1e-6 and e_alb <= 1e-6 and e_ws <= 1e-6 and e_dep <= 1e-6
    assert ended >= 1
    assert int(rs["count"].max()) < cfg["max_steps"]
    assert float(bound.max()) <= oc.IMAGE_BOUND_CAP
    path = os.path.join(HERE, "ngp_occ_render_shaded.pt")
    torch.save(out, path)
    print("wrote ngp_occ_render_shaded.pt", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

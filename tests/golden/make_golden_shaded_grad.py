"""Generate tests/golden/ngp_render_shaded_grad.pt: the REAL reference's gradients through NeRFNetwork.render (renderer_df.py:643 ->
run :310) with shading='lambertian' on the CPU (oracle/ref_loader.py; development container only), on the teacher field and the 256
rays of ngp_render.pt, light normalize((0.3, -0.5, 0.81)), ambient_ratio 0.1, bg_color 1, train mode with perturb=True and the two
draws of make_golden_shaded.py's train case (`noise_seed`, CPU generator):

    loss = (image * g_image).sum() + (weights_sum * g_ws).sum() + lambda_orient * loss_orient      g_image, g_ws: ngp_render.pt's

lambda_orient is chosen here, with the oracle restatement alone (tests/shaded_bwd_common.py: restated_grad), as the power of ten that
brings the orientation term's share of the MLP gradient, |lambda g_orient| / (|g_image_part| + |lambda g_orient|) over the six MLP
tensors, closest to one half; the share must lie in [0.1, 0.9].  The file holds data only: the seeds, the light, lambda and the share,
the six MLP gradients in full, the table gradient as its norm and per-level absolute sums (as ngp_render.pt), the per-sample
d loss / d sigma of the sorted ray, and loss_orient.

    python tests/golden/make_golden_shaded_grad.py"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from oracle import ngp_ref, ref_loader  # noqa: E402

LIGHT = (0.3, -0.5, 0.81)
RATIO = 0.1
BG = 1


def main():
    import shaded_bwd_common as sb
    import shaded_common as sc
    base = torch.load(os.path.join(HERE, "ngp_render.pt"))["teacher"]
    cfg = dict(base["cfg"])
    p = ngp_ref.init_params(bound=4, seed=cfg["seed"], table_std=cfg["table_std"], sigma_bias=cfg["sigma_bias"])
    o, d = sc.golden_rays(cfg)
    assert torch.equal(o, base["rays_o"]) and torch.equal(d, base["rays_d"])
    light = torch.tensor(LIGHT, dtype=torch.float32)
    light = light / light.norm()
    gI, gW = base["g_image"], base["g_ws"]
    noise_seed = 2000 + cfg["seed"]
    uc, uf = sc.golden_draws(noise_seed, o.shape[0])

    # ---- lambda from the restatement: the image part alone, the orientation part alone
    cat = lambda rs: torch.cat([rs["params"][k].grad.flatten() for k in sb.MLP_NAMES])
    g_img = cat(sb.restated_grad(p, o, d, light, RATIO, BG, uc, uf, gI, gW, 0.0))
    g_ori = cat(sb.restated_grad(p, o, d, light, RATIO, BG, uc, uf, torch.zeros_like(gI), torch.zeros_like(gW), 1.0))
    lam = 10.0 ** round(math.log10(float(g_img.norm()) / float(g_ori.norm())))
    share = lam * float(g_ori.norm()) / (float(g_img.norm()) + lam * float(g_ori.norm()))
    print(f"|g image part| {float(g_img.norm()):.4e} |g orient part| {float(g_ori.norm()):.4e} -> lambda {lam:g}, orientation share {share:.3f}")
    assert 0.1 <= share <= 0.9

    # ---- the reference, with grad
    opt = ref_loader.ngp_opt()
    net = ref_loader.reference_ngp()
    net.load_state_dict({k: p[k] for k in net.state_dict().keys()})
    net.train()
    torch.manual_seed(noise_seed)                                     # the reference draws the same two tensors in this order
    r = net.render(o[None], d[None], staged=False, perturb=True, bg_color=BG, ambient_ratio=RATIO, shading='lambertian', light_d=light,
                   force_all_rays=True, **vars(opt))
    loss = (r['image'][0] * gI).sum() + (r['weights_sum'] * gW).sum() + lam * r['loss_orient']
    loss.backward()
    ge = net.encoder.embeddings.grad
    norm, lvl = sb.table_summary(ge, p["encoder.offsets"])

    # ---- d loss / d sigma of the sorted ray is not a leaf of the reference: it comes from the restatement, which must first reproduce the
    # reference's parameter gradients
    rs = sb.restated_grad(p, o, d, light, RATIO, BG, uc, uf, gI, gW, lam)
    for k, v in net.sigma_net.named_parameters():
        rel = float((rs["params"]["sigma_net." + k].grad - v.grad).norm() / v.grad.norm())
        print(f"restatement vs reference {k}: {rel:.2e}")
        assert rel <= 1e-5
    n2, l2 = sb.table_summary(rs["params"]["encoder.embeddings"].grad, p["encoder.offsets"])
    print(f"table norm rel {abs(float(n2) - float(norm)) / float(norm):.2e}, per-level max rel {float(((l2 - lvl).abs() / lvl).max()):.2e}")
    assert torch.allclose(l2, lvl, rtol=1e-5, atol=0)
    rel_o = abs(float(rs["loss_orient"]) - float(r["loss_orient"])) / float(r["loss_orient"])
    assert rel_o <= 1e-6, rel_o

    out = dict(cfg=cfg, light_d=light, ambient_ratio=RATIO, bg_color=BG, epsilon=1e-2, noise_seed=noise_seed, lambda_orient=lam,
               orient_share=share, image=r['image'][0].detach().clone(), weights_sum=r['weights_sum'].detach().clone(),
               loss_orient=r['loss_orient'].detach().clone(),
               grad_mlp={k: v.grad.clone() for k, v in net.sigma_net.named_parameters()},
               grad_table_level_abs=lvl.clone(), grad_table_norm=norm.clone(), dsigma=rs["dsigma"].clone())
    path = os.path.join(HERE, "ngp_render_shaded_grad.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Time the occupancy-grid EVALUATION render (cuda_ray=True, eval mode): one fused launch (sf_ngp_render_occ_eval, or with
--shading lambertian sf_ngp_render_occ_eval_shaded, eight lanes per ray) instead of the reference's host loop of march / network /
composite rounds.
usage: occ_eval_time.py [--shading albedo|lambertian] [--side 256] [--repeats 20] [--passes 2] [--scene field|ball]
--shading albedo (default) measures as the tool always did: warm-up, then the mean of --repeats back-to-back renders with one
synchronise at the end, so its line stays comparable with the earlier logs (profiles/r02_occ_eval.log).
--shading lambertian reports, per view of side x side rays: (a) the shaded launch, (b) the albedo launch, (c) the reference-style round
loop composed from this library's own entry points (march_rays -> point_attributes -> torch shading -> composite_rays, with its host
read of the alive count per round); warm-up, then the median of --repeats runs, each synchronised, the three alternating over
--passes passes (one line per pass: their difference is the spread); the total number of samples
composited and the time per 1 000 field evaluations (7 per sample shaded, 1 per sample albedo).
--scene field (default): a weak default-like field and the grid update_extra_state gives it -- nearly every sample is skipped, the
render is a march.  --scene ball: a dense field (table_std 3, sigma_bias 1) behind an analytic ball bitfield (radius 1.3): the rays that
hit it composite ~100 samples each, the render is field evaluations."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import torch
from oracle import ngp_ref
from sparsefusion_amd import _lib, mesh, raymarching
from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
ap = argparse.ArgumentParser()
ap.add_argument("--shading", default="albedo", choices=("albedo", "lambertian"))
ap.add_argument("--side", type=int, default=256)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--scene", default="field", choices=("field", "ball"))
args = ap.parse_args()
dev = "cuda:0"
opt = get_default_torch_ngp_opt()
opt.cuda_ray = True
ball = args.scene == "ball"
p = ngp_ref.init_params(bound=4, seed=1, table_std=3.0 if ball else 0.5, sigma_bias=1.0 if ball else -3.0)
net = NeRFNetwork(opt)
sd = net.state_dict()
sd.update({k: p[k] for k in p if k in sd})
net.load_state_dict(sd)
net = net.to(dev).train()
if ball:                                                            # 1 inside the ball, per cascade, in Morton order
    Hg = net.grid_size
    cells = raymarching.morton3D_invert(torch.arange(Hg ** 3, dtype=torch.int32, device=dev)).float()
    centre = torch.tensor([0.2, -0.1, 0.3], device=dev)
    grid = torch.stack([((((cells + 0.5) / Hg * 2 - 1) * min(2.0 ** c, net.bound) - centre).norm(dim=-1) < 1.3).float()
                        for c in range(net.cascade)])
    net.density_bitfield.copy_(raymarching.packbits(grid, 0.5))
else:
    for _ in range(3):
        net.update_extra_state()
net.eval()
o, d = ngp_ref.circle_rays(args.side, view=3)
o, d = o[None].to(dev), d[None].to(dev)
light = torch.tensor([0.3, -0.5, 0.81], device=dev)
light = light / light.norm()
ratio = torch.tensor(0.1, device=dev)
kw = dict(vars(opt))


def timed(fn, warm=3):
    with torch.no_grad():
        for _ in range(warm):
            r = fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), r


def albedo():
    return net.render(o, d, staged=False, perturb=False, bg_color=0, shading='albedo', **kw)


def shaded():
    return net.render(o, d, staged=False, perturb=False, bg_color=0, shading='lambertian', light_d=light, ambient_ratio=0.1, **kw)


def round_loop():
    """renderer_df.py:523-556 with shading='lambertian', on this library's entry points.  A round restarts the marcher from
    rays_t = near + the composited gaps, which on a few rays is an ulp or two away from the marcher's own t: the image differs from
    the one-launch render's by that, amplified by the field's finest cells"""
    oo, dd = o[0].contiguous(), d[0].contiguous()
    N = oo.shape[0]
    nears, fars = raymarching.near_far_from_aabb(oo, dd, net.aabb_infer)
    ws, depth, image = (torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, 3, device=dev))
    alive, rays_t = torch.arange(N, dtype=torch.int32, device=dev), nears.clone()
    step, max_steps = 0, kw["max_steps"]
    while step < max_steps:
        n_alive = alive.shape[0]                                    # the host read of every round (a device-to-host sync)
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        x, _, dl = raymarching.march_rays(n_alive, n_step, alive, rays_t, oo, dd, net.bound, net.density_bitfield, net.cascade,
                                          net.grid_size, nears, fars, 128, False, kw["dt_gamma"], max_steps)
        at = mesh.point_attributes(net, x, 1e-2, grad=False)
        n = at["normal"]                                        # elementwise, left to right: the kernel's arithmetic
        dot = (n[:, 0] * -light[0] + n[:, 1] * -light[1]) + n[:, 2] * -light[2]
        lam = ratio + (1 - ratio) * dot.clamp(min=0)
        raymarching.composite_rays(n_alive, n_step, alive, rays_t, at["sigma"], at["albedo"] * lam.unsqueeze(-1), dl, ws, depth, image,
                                   kw.get("T_thresh", 1e-4))
        alive = alive[alive >= 0]
        step += n_step
    return dict(image=image, weights_sum=ws)


def n_samples():
    """samples composited per ray, from the shaded entry"""
    oo, dd = o[0].contiguous(), d[0].contiguous()
    N = oo.shape[0]
    nears, fars = raymarching.near_far_from_aabb(oo, dd, net.aabb_infer)
    f32 = dict(dtype=torch.float32, device=dev)
    ws, dep, img, cnt = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, 3, **f32), torch.zeros(N, dtype=torch.int32, device=dev)
    prm = [q.detach().contiguous() for q in net._field_params()]
    f = net._field_handle().struct(prm)
    rc = _lib.lib().sf_ngp_render_occ_eval_shaded(C.byref(f), _lib.ptr(oo), _lib.ptr(dd), _lib.ptr(nears), _lib.ptr(fars),
                                                  _lib.ptr(net.density_bitfield), float(kw["dt_gamma"]), int(kw["max_steps"]),
                                                  int(net.cascade), int(net.grid_size), None, float(kw.get("T_thresh", 1e-4)), N,
                                                  _lib.ptr(light), 0.1, 1e-2, _lib.ptr(ws), _lib.ptr(dep), _lib.ptr(img), None,
                                                  _lib.ptr(cnt), _lib.stream_ptr())
    _lib.check(rc, "ngp_render_occ_eval_shaded")
    return int(cnt.sum())


side = args.side
if args.shading == "albedo":                                        # as before --shading: the mean of back-to-back renders, one synchronise
    with torch.no_grad():
        for _ in range(3):
            r = albedo()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.repeats):
            r = albedo()
        torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.repeats * 1e3
    print(f"occupancy-grid eval render {side}x{side} rays: {ms:.3f} ms per view (one launch + near/far), mean opacity {float(r['weights_sum'].mean()):.4f}, "
          f"occupied cells {int(sum(bin(int(b)).count('1') for b in net.density_bitfield.cpu().tolist()))}")
else:
    total = n_samples()
    for k in range(args.passes):
        a, a_min, ra = timed(shaded)
        b, b_min, rb = timed(albedo)
        c, c_min, rc_ = timed(round_loop)
        print(f"occupancy-grid eval render {side}x{side} rays, scene {args.scene}, pass {k}, median of {args.repeats} (min): (a) shaded launch {a:.3f} ({a_min:.3f}) ms, "
              f"(b) albedo launch {b:.3f} ({b_min:.3f}) ms, (c) round loop of march_rays / point_attributes / composite_rays {c:.3f} "
              f"({c_min:.3f}) ms; a / b = {a / b:.2f}, c / a = {c / a:.2f}; per 1 000 field evaluations: shaded "
              f"{a * 1e3 / (7 * total) * 1e3:.3f} us, albedo {b * 1e3 / total * 1e3:.3f} us")
    err = float((ra['image'][0] - rc_['image']).abs().max())
    print(f"  samples composited {total} ({total / side / side:.1f} per ray), mean opacity {float(ra['weights_sum'].mean()):.4f}; "
          f"max |image (a) - (c)| {err:.2e}")

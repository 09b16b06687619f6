"""Time the fused NGP render (forward, forward+backward) at the BASELINE size: 128x128 rays, 64+64 samples.
--shading lambertian adds, after the default output: the shaded render (sf_ngp_render_shaded_forward), the albedo forward at the same
size, and the composed route (albedo forward + sf_ngp_point_attrs over the sorted points + torch glue for the weights and the sums),
each the median of 5 torch-event timings after a warm-up.
--shading lambertian --backward times instead the DIFFERENTIABLE shaded render, forward + backward of image.mean() + weights_sum.mean()
+ loss_orient: the fused route (run(shading='lambertian', shading_backward=True): sf_ngp_render_shaded_forward_train / _backward), the
albedo render's forward + backward at the same size, and the composed route -- the albedo forward for the sorted ray, then
NeRFNetwork.forward(x, d, l, ratio, 'lambertian') under autograd on the sorted points (seven field evaluations through the grid-encode
op) and torch compositing.
--bwd-pipe 0|1 selects the kernel of the cached field backward (renderer._FIELD_BWD_PIPE) instead of the default.
--feat-cache 0|1 sets renderer._FEAT_CACHE: 0 = no field cache, the backward re-gathers the features (k_ngp_field_bwd_mfma).
--log2-hashmap N --gridtype hash|tiled swaps the encoder for one of 2^N rows per level (random table): with N = 20 the table is outside the
binned scatter and the backward takes k_ngp_scatter + k_ngp_scatter_fine (csrc/ngp_scatter.h), which the default teacher field never launches."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ngp_ref  # noqa: E402  (parameter initialiser only)
from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt  # noqa: E402

if "--bwd-pipe" in sys.argv:
    from sparsefusion_amd.nerf import renderer as _R
    _R._FIELD_BWD_PIPE = sys.argv[sys.argv.index("--bwd-pipe") + 1] == "1"
    print(f"field backward  : {'k_ngp_field_bwd_pipe' if _R._FIELD_BWD_PIPE else 'k_ngp_field_bwd_mfma'}")
if "--feat-cache" in sys.argv:
    from sparsefusion_amd.nerf import renderer as _R
    _R._FEAT_CACHE = sys.argv[sys.argv.index("--feat-cache") + 1] == "1"
    print(f"field cache     : {'kept by the forward' if _R._FEAT_CACHE else 'none (the backward re-gathers the features)'}")
dev = "cuda:0"
p = ngp_ref.init_params(bound=4, seed=1, table_std=0.5, sigma_bias=-3.0)
net = NeRFNetwork(get_default_torch_ngp_opt())
net.load_state_dict({k: p[k] for k in net.state_dict().keys()})
net = net.to(dev).train()
if "--log2-hashmap" in sys.argv:
    from sparsefusion_amd.gridencoder import GridEncoder
    log2_rows = int(sys.argv[sys.argv.index("--log2-hashmap") + 1])
    gridtype = sys.argv[sys.argv.index("--gridtype") + 1] if "--gridtype" in sys.argv else "hash"
    enc = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=log2_rows,
                      desired_resolution=2048 * net.bound, gridtype=gridtype, align_corners=False).to(dev)
    with torch.no_grad():
        enc.embeddings.copy_((torch.rand(enc.embeddings.shape, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev))
    net.encoder, net._handle = enc, None
    print(f"encoder         : {gridtype}, 2^{log2_rows} rows per level")
o, d = ngp_ref.circle_rays(128, view=7)
o, d = o[None].to(dev), d[None].to(dev)
kw = dict(staged=False, perturb=True, bg_color=0, shading='albedo', **vars(net.opt))


def run(backward, iters):
    torch.cuda.synchronize()
    t = time.time()
    for _ in range(iters):
        net.zero_grad(set_to_none=True)
        with torch.set_grad_enabled(backward):
            r = net.render(o, d, **kw)
            if backward:
                (r["image"].mean() + r["weights_sum"].mean()).backward()
    torch.cuda.synchronize()
    return (time.time() - t) / iters * 1e3


run(True, 3)
print(f"render fwd      : {run(False, 20):.3f} ms")
print(f"render fwd+bwd  : {run(True, 20):.3f} ms")


def shaded_times():
    import ctypes as C
    from sparsefusion_amd import _lib, mesh
    light = torch.tensor([0.3, -0.5, 0.81], device=dev)
    light = light / light.norm()
    ratio, T = 0.1, net.opt.num_steps
    of, df = o[0].contiguous(), d[0].contiguous()
    N = of.shape[0]
    skw = dict(kw, perturb=False)

    def shaded():
        return net.render(o, d, **dict(skw, shading='lambertian', light_d=light, ambient_ratio=ratio))

    def albedo():
        return net.render(o, d, **skw)

    def composed():
        # the albedo forward through the C ABI (the sorted ray is not part of run's result), then the point attributes and torch
        f32 = dict(dtype=torch.float32, device=dev)
        lin, det = net._table(T, of.device)
        params = [q.detach().contiguous() for q in net._field_params()]
        f = net._field_handle().struct(params)
        lib = _lib.lib()
        nears, fars, depth, ws = (torch.empty(N, **f32) for _ in range(4))
        z_s, sig_s, rgb_s, image = torch.empty(N, 2 * T, **f32), torch.empty(N, 2 * T, **f32), torch.empty(N, 2 * T, 3, **f32), torch.empty(N, 3, **f32)
        wbytes = lib.sf_ngp_render_forward_workspace_bytes(N, T)
        work = torch.empty(wbytes // 4, **f32)
        u_fine = torch.rand(N, T, device=dev)                          # train mode: the inverse-CDF draw
        _lib.check(lib.sf_ngp_render_forward(C.byref(f), _lib.ptr(of), _lib.ptr(df), _lib.ptr(net.aabb_train), N, T, float(net.min_near),
                                             _lib.ptr(lin), None, _lib.ptr(u_fine), T, 0.0, _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(z_s),
                                             _lib.ptr(sig_s), _lib.ptr(rgb_s), _lib.ptr(image), _lib.ptr(depth), _lib.ptr(ws), None,
                                             _lib.ptr(work), wbytes, _lib.stream_ptr()), "ngp_render_forward")
        x = torch.min(torch.max(of[:, None] + df[:, None] * z_s[..., None], net.aabb_train[:3]), net.aabb_train[3:])
        n = mesh.point_attributes(net, x.view(-1, 3), 1e-2, sigma=False, albedo=False, grad=False)["normal"].view(N, 2 * T, 3)
        col = rgb_s * (ratio + (1 - ratio) * (n @ -light).clamp(min=0)).unsqueeze(-1)
        deltas = torch.cat([z_s[:, 1:] - z_s[:, :-1], ((fars - nears) / T)[:, None]], -1)
        alphas = 1 - torch.exp(-deltas * sig_s)
        w = alphas * torch.cumprod(torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-15], -1), -1)[:, :-1]
        img = (w[..., None] * col).sum(-2) + (1 - w.sum(-1))[:, None] * 0.0
        return img, (w[..., None] * n).sum(-2), (w * (n * df[:, None]).sum(-1).clamp(min=0) ** 2).mean()

    def median_ms(fn):
        with torch.no_grad():
            fn()
            ts = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
        return sorted(ts)[2]

    print(f"shaded render   : {median_ms(shaded):.3f} ms")
    print(f"albedo forward  : {median_ms(albedo):.3f} ms")
    print(f"composed shaded : {median_ms(composed):.3f} ms")


def shaded_backward_times():
    import ctypes as C
    from sparsefusion_amd import _lib
    light = torch.tensor([0.3, -0.5, 0.81], device=dev)
    light = light / light.norm()
    ratio, T = 0.1, net.opt.num_steps
    of, df = o[0].contiguous(), d[0].contiguous()
    N = of.shape[0]

    def fused():
        net.zero_grad(set_to_none=True)
        r = net.render(o, d, **dict(kw, shading='lambertian', light_d=light, ambient_ratio=ratio, shading_backward=True))
        (r["image"].mean() + r["weights_sum"].mean() + r["loss_orient"]).backward()

    def albedo():
        net.zero_grad(set_to_none=True)
        r = net.render(o, d, **kw)
        (r["image"].mean() + r["weights_sum"].mean()).backward()

    def composed():
        net.zero_grad(set_to_none=True)
        f32 = dict(dtype=torch.float32, device=dev)
        lin, det = net._table(T, of.device)
        params = [q.detach().contiguous() for q in net._field_params()]
        f = net._field_handle().struct(params)
        lib = _lib.lib()
        nears, fars, depth, ws = (torch.empty(N, **f32) for _ in range(4))
        z_s, sig_s, rgb_s, image = torch.empty(N, 2 * T, **f32), torch.empty(N, 2 * T, **f32), torch.empty(N, 2 * T, 3, **f32), torch.empty(N, 3, **f32)
        wbytes = lib.sf_ngp_render_forward_workspace_bytes(N, T)
        work = torch.empty(wbytes // 4, **f32)
        u_c, u_fine = torch.rand(N, T, device=dev), torch.rand(N, T, device=dev)
        _lib.check(lib.sf_ngp_render_forward(C.byref(f), _lib.ptr(of), _lib.ptr(df), _lib.ptr(net.aabb_train), N, T, float(net.min_near),
                                             _lib.ptr(lin), _lib.ptr(u_c), _lib.ptr(u_fine), T, 0.0, _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(z_s),
                                             _lib.ptr(sig_s), _lib.ptr(rgb_s), _lib.ptr(image), _lib.ptr(depth), _lib.ptr(ws), None,
                                             _lib.ptr(work), wbytes, _lib.stream_ptr()), "ngp_render_forward")
        x = torch.min(torch.max(of[:, None] + df[:, None] * z_s[..., None], net.aabb_train[:3]), net.aabb_train[3:])
        dirs = df[:, None].expand(N, 2 * T, 3)
        sigma, col, n = net(x.view(-1, 3), dirs.reshape(-1, 3), light, ratio=ratio, shading='lambertian')
        sigma, col, n = sigma.view(N, 2 * T), col.view(N, 2 * T, 3), n.view(N, 2 * T, 3)
        deltas = torch.cat([z_s[:, 1:] - z_s[:, :-1], ((fars - nears) / T)[:, None]], -1)
        alphas = 1 - torch.exp(-deltas * sigma)
        w = alphas * torch.cumprod(torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-15], -1), -1)[:, :-1]
        img = (w[..., None] * col).sum(-2)
        orient = (w.detach() * (n * dirs).sum(-1).clamp(min=0) ** 2).mean()
        (img.mean() + w.sum(-1).mean() + orient).backward()

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts)[2]

    print(f"shaded fwd+bwd  : {median_ms(fused):.3f} ms   (fused: sf_ngp_render_shaded_forward_train + sf_ngp_render_shaded_backward)")
    print(f"albedo fwd+bwd  : {median_ms(albedo):.3f} ms")
    print(f"composed fwd+bwd: {median_ms(composed):.3f} ms   (albedo forward + NeRFNetwork.forward('lambertian') under autograd + torch compositing)")


if "--shading" in sys.argv and sys.argv[sys.argv.index("--shading") + 1:][:1] == ["lambertian"]:
    if "--backward" in sys.argv:
        shaded_backward_times()
    else:
        shaded_times()

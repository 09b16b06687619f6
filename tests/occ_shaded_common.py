"""Shared pieces of the shaded occupancy-grid evaluation render's tests (sf_ngp_render_occ_eval_shaded;
sparsefusion_amd/csrc/ngp_occ_shade.h): the scenes, the CPU restatement of run_cuda(shading='lambertian') in eval mode composed from
the C oracle's march / composite and point_attrs_common, the bounds the density tolerances imply for it, the route composed on the GPU
from entry points that are already pinned, and the ctypes harness of tests/hostemu/occ_shade_emu.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import point_attrs_common as pc
from ngp_common import log2_scale
from occ_common import BOUND, CASCADE, H, ball_bitfield, camera_rays
from oracle import ngp_native, ngp_ref

EPS = 1e-2                                     # the reference's fixed finite-difference step (network_grid.py:91)
CFG = dict(seed=1, table_std=3.0, sigma_bias=1.0, n_side=16, max_steps=256, dt_gamma=0.0, T_thresh=1e-4, min_near=0.2)
LIGHT = (0.3, -0.5, 0.81)
LIGHT2 = (-0.7, 0.2, -0.4)
RATIO, BG = 0.1, 1
IMAGE_BOUND_CAP = 1e-2
SMALL_N = (1, 7, 8, 9, 33)                     # a lone group, a wave's last group, a second wave, a second workgroup
SMALL_RADIUS, SMALL_STEPS = 2.0, 64


def unit(v):
    l = torch.tensor(v, dtype=torch.float32)
    return l / l.norm()


def params():
    return ngp_ref.init_params(bound=4, seed=CFG["seed"], table_std=CFG["table_std"], sigma_bias=CFG["sigma_bias"])


def near_far(o, d, min_near=CFG["min_near"]):
    aabb = torch.tensor([-BOUND, -BOUND, -BOUND, BOUND, BOUND, BOUND])
    nears, fars = torch.empty(o.shape[0]), torch.empty(o.shape[0])
    ngp_native.near_far_from_aabb(o.contiguous(), d.contiguous(), aabb, o.shape[0], min_near, nears, fars)
    return nears, fars


def golden_scene():
    """the 256 rays and the analytic ball bitfield of tests/golden/ngp_occ_render_shaded.pt"""
    _, bits, _ = ball_bitfield()
    o, d = camera_rays(CFG["n_side"])
    nears, fars = near_far(o, d)
    return dict(bits=bits, o=o, d=d, nears=nears, fars=fars, max_steps=CFG["max_steps"])


_SMALL_ORDER = [54, 248, 200, 7, 120, 143, 195, 100, 33] + [i for i in range(4, 256, 8) if i != 100][:24]
_SMALL_ORDER += [i for i in range(256) if i not in _SMALL_ORDER]                  # a fixed permutation of the 16 x 16 camera


def small_scene(N, max_steps=SMALL_STEPS):
    """The first N rays of a fixed order of the 16 x 16 camera, with UNIT directions, against the radius-2 ball: a ray covers
    2 sqrt(3) = 3.46 in max_steps steps of dt_min and the ball's longest chord is 4, so the rays through the middle (the first
    one) are capped at max_steps; the second one misses the ball; others graze it."""
    _, bits, _ = ball_bitfield(radius=SMALL_RADIUS)
    o, d = camera_rays(16)
    idx = torch.tensor(_SMALL_ORDER[:N])
    o, d = o[idx].clone(), d[idx].clone()
    d = d / d.norm(dim=-1, keepdim=True)
    nears, fars = near_far(o, d)
    return dict(bits=bits, o=o.contiguous(), d=d.contiguous(), nears=nears, fars=fars, max_steps=max_steps)


# ------------------------------------------------------------------------------------------------------------------ the oracle
def oracle_march(sc, dt_gamma=0.0):
    """one round of the C oracle's march_rays with n_step = max_steps -> xyzs [N, S, 3], deltas [N, S, 2], per-ray count"""
    N, S = sc["o"].shape[0], sc["max_steps"]
    alive, rays_t = torch.arange(N, dtype=torch.int32), sc["nears"].clone()
    x, dr, dl = torch.zeros(N * S, 3), torch.zeros(N * S, 3), torch.zeros(N * S, 2)
    ngp_native.march_rays(N, S, alive, rays_t, sc["o"], sc["d"], BOUND, dt_gamma, S, CASCADE, H, sc["bits"], sc["nears"], sc["fars"],
                          x, dr, dl, torch.zeros(N))
    return x.view(N, S, 3), dl.view(N, S, 2), (dl.view(N, S, 2)[..., 0] != 0).sum(1)


def oracle_composite(sc, sigmas, rgbs, deltas, T_thresh):
    N, S = sc["o"].shape[0], sc["max_steps"]
    alive, rays_t = torch.arange(N, dtype=torch.int32), sc["nears"].clone()
    ws, depth, image = torch.zeros(N), torch.zeros(N), torch.zeros(N, 3)
    ngp_native.composite_rays(N, S, T_thresh, alive, rays_t, sigmas.reshape(-1).contiguous(), rgbs.reshape(-1, 3).contiguous(),
                              deltas.reshape(-1, 2).contiguous(), ws, depth, image)
    return ws, depth, image


def restated(p, sc, light, ratio, T_thresh, dt_gamma=0.0):
    """run_cuda(shading='lambertian'), eval mode (renderer_df.py:523-556 with network_grid.py:129-153), on the CPU: the samples of one
    march_rays round with n_step = max_steps (a ray's samples do not depend on the reference's batching into rounds), the field and
    its finite-difference normals as point_attrs_common composes them, torch float32 shading, the C oracle's composite_rays.
    image / normal_image without background, depth un-normalised (what the C entry returns)."""
    with torch.no_grad():
        x, dl, count = oracle_march(sc, dt_gamma)
        N, S = x.shape[:2]
        used = dl[..., 0] != 0
        xu = x[used].contiguous()
        ref = pc.oracle_attrs(p, xu, EPS)
        normal_u = torch.from_numpy(pc.np_normal(ref["grad"].numpy()))
        lam = ratio + (1 - ratio) * (normal_u @ -light).clamp(min=0)
        sigma, albedo, color, normal = torch.zeros(N, S), torch.zeros(N, S, 3), torch.zeros(N, S, 3), torch.zeros(N, S, 3)
        sigma[used], albedo[used], color[used], normal[used] = ref["sigma"], ref["albedo"], ref["albedo"] * lam.unsqueeze(-1), normal_u
        ws, depth, image = oracle_composite(sc, sigma, color, dl, T_thresh)
        ws_a, depth_a, image_a = oracle_composite(sc, sigma, albedo, dl, T_thresh)
        _, _, nimg = oracle_composite(sc, sigma, normal, dl, T_thresh)
        with np.errstate(divide="ignore", invalid="ignore"):
            ru = np.linalg.norm(pc.grad_bound(ref, EPS), axis=1) / np.linalg.norm(ref["grad"].double().numpy(), axis=1)
        ru[np.isnan(ru)] = np.inf
        r = np.zeros((N, S))
        r[used.numpy()] = ru
        # the compositor's weights in float64: w_i = alpha_i T_i, the sample at which T_i < T_thresh is the last one
        alpha = 1.0 - torch.exp(-sigma.double() * dl[..., 0].double())
        T = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=torch.float64), 1.0 - alpha[:, :-1]], 1), 1)
        keep = used & torch.cat([torch.ones(N, 1, dtype=torch.bool), T[:, :-1] >= T_thresh], 1)
        w = (alpha * T * keep).numpy()
    return dict(x=x, deltas=dl, count=count, used=used, sigma=sigma, albedo=albedo, normal=normal, image=image, depth=depth,
                weights_sum=ws, normal_image=nimg, image_albedo=image_a, depth_albedo=depth_a, weights_sum_albedo=ws_a,
                n_samples=keep.sum(1), weights=w, r=r, light=light, ratio=ratio, T_thresh=T_thresh)


def finish(sc, image, depth, ws, bg=BG):
    """what run_cuda returns from the entry's outputs: background mixed in, depth normalised (renderer_df.py:566-575)"""
    return image + (1 - ws).unsqueeze(-1) * bg, torch.clamp(depth - sc["nears"], min=0) / (sc["fars"] - sc["nears"])


def delta(rs):
    """per sample: how far the density tolerances let the unit normal move -- 2 r + 1e-6 (test_point_attrs_cpu.py), at most 2"""
    return np.minimum(2.0, 2.0 * rs["r"] + 1e-6)


def wdelta(rs):
    return (rs["weights"] * delta(rs)).sum(axis=1)


def image_bound(rs):
    """[N]: 2e-5 + T_thresh + (1 - ratio) sum_i w_i delta_i.  albedo <= 1 and |l| = 1, so the lambertian factor of a sample moves by at
    most (1 - ratio) delta_i; 2e-5 covers the albedo / weight tolerances of the albedo render (shaded_common.image_bound); T_thresh
    covers a ray whose last sample falls on the other side of the threshold: what it adds is at most w <= T < T_thresh."""
    return 2e-5 + rs["T_thresh"] + (1.0 - rs["ratio"]) * wdelta(rs)


# Bounds of the other outputs against the restatement, from the same tolerances.  A relative density error e = 2e-5 (SIGMA_RTOL) moves
# w_i = alpha_i T_i by at most w_i e (1 + tau_i), tau_i the optical depth in front of and in sample i (d alpha / alpha <= e, d T / T <=
# e tau); sum_i w_i (1 + tau_i) <= int_0^inf e^-tau (1 + tau) d tau = 2, so sum_i |d w_i| <= 4e-5; 1e-5 on top for the float32 sums (at
# most 256 terms of magnitude <= 1) and exp.  A threshold flip adds or removes one sample of weight < T_thresh.
def weights_bound(rs):
    return 5e-5 + rs["T_thresh"]


def depth_bound(rs, fars):
    """depth = sum w_i t_i is un-normalised, t_i <= far"""
    return (5e-5 + rs["T_thresh"]) * fars.double().numpy() + 1e-5


def normal_bound(rs):
    """sum w n: |n| <= 1 moves by delta_i per sample, the weights as above"""
    return 5e-5 + rs["T_thresh"] + wdelta(rs)


# ------------------------------------------------------------------------------------------------------------- composed GPU route
def composed_gpu(net, sc_dev, light, ratio, T_thresh, dt_gamma=0.0, noises=None):
    """The reference-style route from entry points that are already pinned, ONE round at n_step = max_steps: raymarching.march_rays,
    mesh.point_attributes on its points, shading in torch elementwise float32 (the dot product left to right, one rounding per
    operation), raymarching.composite_rays once with the shaded colour and once with the normals as rgbs (sum w n).
    -> weights_sum, depth, image, normal_image, march count per ray (device tensors)"""
    from sparsefusion_amd import mesh, raymarching
    o, d, nears, fars, bits, S = (sc_dev[k] for k in ("o", "d", "nears", "fars", "bits", "max_steps"))
    N, dev = o.shape[0], o.device
    f32 = dict(dtype=torch.float32, device=dev)
    alive, rays_t = torch.arange(N, dtype=torch.int32, device=dev), nears.clone()
    nz = torch.zeros(N, **f32) if noises is None else noises
    x, _, dl = raymarching.march_rays(N, S, alive, rays_t, o, d, BOUND, bits, CASCADE, H, nears, fars, -1, noises is not None,
                                      dt_gamma, S, noises=nz)
    at = mesh.point_attributes(net, x, EPS, grad=False)
    n, l = at["normal"], light.to(dev)
    dot = (n[:, 0] * -l[0] + n[:, 1] * -l[1]) + n[:, 2] * -l[2]
    rt = torch.tensor(ratio, **f32)
    lam = rt + (1 - rt) * dot.clamp(min=0)
    color = at["albedo"] * lam.unsqueeze(-1)
    outs = []
    for rgbs in (color, n):
        alive, rays_t = torch.arange(N, dtype=torch.int32, device=dev), nears.clone()
        ws, depth, image = torch.zeros(N, **f32), torch.zeros(N, **f32), torch.zeros(N, 3, **f32)
        raymarching.composite_rays(N, S, alive, rays_t, at["sigma"], rgbs.contiguous(), dl, ws, depth, image, T_thresh)
        outs.append((ws, depth, image))
    return outs[0][0], outs[0][1], outs[0][2], outs[1][2], (dl.view(N, S, 2)[..., 0] != 0).sum(1)


def gpu_entry(net, sc_dev, light, ratio, T_thresh, dt_gamma=0.0, noises=None, eps=EPS, normal=True, count=True, shaded=True):
    """sf_ngp_render_occ_eval_shaded (or, shaded=False, sf_ngp_render_occ_eval) on device tensors; outputs pre-filled with NaN /
    0xFFFFFFFF; None for skipped ones"""
    from sparsefusion_amd import _lib
    o, d, nears, fars, bits, S = (sc_dev[k] for k in ("o", "d", "nears", "fars", "bits", "max_steps"))
    N, dev = o.shape[0], o.device
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)      # noqa: E731
    out = dict(weights_sum=nan(N), depth=nan(N), image=nan(N, 3), normal_image=nan(N, 3) if (normal and shaded) else None,
               n_samples=torch.full((N,), -1, dtype=torch.int32, device=dev) if (count and shaded) else None)
    prm = [q.detach().contiguous() for q in net._field_params()]
    f = net._field_handle().struct(prm)
    head = (C.byref(f), _lib.ptr(o), _lib.ptr(d), _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(bits), float(dt_gamma), int(S), CASCADE, H,
            _lib.ptr(noises), float(T_thresh), N)
    tail = (_lib.ptr(out["weights_sum"]), _lib.ptr(out["depth"]), _lib.ptr(out["image"]))
    if shaded:
        l = light.to(dev).contiguous()
        rc = _lib.lib().sf_ngp_render_occ_eval_shaded(*head, _lib.ptr(l), float(ratio), float(eps), *tail, _lib.ptr(out["normal_image"]),
                                                      _lib.ptr(out["n_samples"]), _lib.stream_ptr())
    else:
        rc = _lib.lib().sf_ngp_render_occ_eval(*head, *tail, _lib.stream_ptr())
    _lib.check(rc, "render_occ_eval")
    return out


def make_net(p, dev):
    """an eval-mode cuda_ray network holding the oracle's parameters; the caller loads the bitfield"""
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    opt = get_default_torch_ngp_opt()
    opt.cuda_ray = True
    net = NeRFNetwork(opt)
    sd = net.state_dict()
    sd.update({k: p[k] for k in p if k in sd})
    net.load_state_dict(sd)
    return net.to(dev).eval(), opt


def to_dev(sc, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.items()}


# ---------------------------------------------------------------------------------------------------------------- host emulation
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_SO = os.path.join(_HERE, "_build", "libocc_shade_emu.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_handle = None


def emu_available():
    return os.path.exists(CLANG)


def _emu():
    global _handle
    if _handle is None:
        csrc = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
        deps = [os.path.join(_HERE, f) for f in ("occ_shade_emu.cpp", "ngp_host.cpp", "ngp_emu_common.h", "hip_emu.h")] + \
               [os.path.join(csrc, f) for f in ("ngp_occ_shade.h", "occ_marcher.h", "ngp_point_attrs.h", "ngp_device.h", "sf_dev.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call([CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + _HERE, "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-Wno-source-uses-openmp", "-ffp-contract=off", deps[0], "-o", _SO,
                                   "-lpthread"])
        _handle = C.CDLL(_SO)
        for name in ("emu_occ_eval_shaded", "emu_occ_eval"):
            getattr(_handle, name).restype = None
    return _handle


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _emu_head(p, sc, dt_gamma, T_thresh, noises):
    offs = p["encoder.offsets"].contiguous()
    w = [p[f"sigma_net.net.{i}.{k}"].contiguous() for i in range(3) for k in ("weight", "bias")]
    keep = [sc[k].contiguous() for k in ("o", "d", "nears", "fars", "bits")] + [offs, noises] + w
    args = [_p(p["encoder.embeddings"]), _p(offs), C.c_uint32(offs.numel() - 1), C.c_float(log2_scale()), C.c_uint32(16), C.c_uint32(1),
            *[_p(t) for t in w], C.c_float(BOUND), *[_p(t) for t in keep[:5]], C.c_float(dt_gamma), C.c_uint32(sc["max_steps"]),
            C.c_uint32(CASCADE), C.c_uint32(H), _p(noises), C.c_float(T_thresh), C.c_uint32(sc["o"].shape[0])]
    return args, keep


def emu_shaded(p, sc, light, ratio, T_thresh, dt_gamma=0.0, noises=None, eps=EPS, normal=True, count=True):
    """k_render_occ_eval_shaded on CPU fibers; outputs pre-filled with NaN / -1; None for skipped ones"""
    N = sc["o"].shape[0]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32)      # noqa: E731
    out = dict(weights_sum=nan(N), depth=nan(N), image=nan(N, 3), normal_image=nan(N, 3) if normal else None,
               n_samples=torch.full((N,), -1, dtype=torch.int32) if count else None)
    args, keep = _emu_head(p, sc, dt_gamma, T_thresh, noises)
    l = light.contiguous().float()
    _emu().emu_occ_eval_shaded(*args, _p(l), C.c_float(ratio), C.c_float(eps),
                               *[_p(out[k]) for k in ("weights_sum", "depth", "image", "normal_image", "n_samples")])
    del keep
    return out


def emu_albedo(p, sc, T_thresh, dt_gamma=0.0, noises=None):
    """the restatement of k_render_occ_eval in occ_shade_emu.cpp"""
    N = sc["o"].shape[0]
    out = dict(weights_sum=torch.full((N,), float("nan")), depth=torch.full((N,), float("nan")), image=torch.full((N, 3), float("nan")))
    args, keep = _emu_head(p, sc, dt_gamma, T_thresh, noises)
    _emu().emu_occ_eval(*args, *[_p(out[k]) for k in ("weights_sum", "depth", "image")])
    del keep
    return out

"""Shared pieces of the shaded-render tests (sf_ngp_render_shaded_forward; sparsefusion_amd/csrc/ngp_shade.h): the oracle
restatement of NeRFRenderer.run(shading='lambertian') composed from ngp_ref.render_run + point_attrs_common, the bounds the density
tolerances imply for it, the numpy float32 restatements of the kernels' formulas, and the ctypes harness of
tests/hostemu/shade_emu.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import point_attrs_common as pc
from ngp_common import BOUND, log2_scale
from oracle import ngp_ref

EPS = 1e-2                                     # the reference's fixed finite-difference step (network_grid.py:91)
F32 = np.float32


def golden_rays(cfg):
    """the 256 rays of tests/golden/ngp_render.pt (one misses the box), re-derived from its cfg"""
    o, d = ngp_ref.circle_rays(16, view=cfg["view"], unit_dir=cfg["unit_dir"])
    o[5] = torch.tensor([20.0, 20.0, 20.0]); d[5] = torch.tensor([1.0, 0.0, 0.0])
    return o, d


def small_rays(N):
    """N rays spread over the golden teacher view; for N > 1 the last but one misses the box"""
    o, d = ngp_ref.circle_rays(16, view=3)
    idx = torch.linspace(40, 215, N).round().long()
    o, d = o[idx].clone(), d[idx].clone()
    if N > 1:
        o[N - 2] = torch.tensor([20.0, 20.0, 20.0]); d[N - 2] = torch.tensor([1.0, 0.0, 0.0])
    return o.contiguous(), d.contiguous()


def golden_draws(noise_seed, N, T=64):
    """the reference's two draws of a perturbed training render with a given light, from the CPU generator"""
    g = torch.Generator().manual_seed(noise_seed)
    return torch.rand(N, T, generator=g), torch.rand(N, T, generator=g)


def sorted_points(o, d, z, aabb):
    """min(max(o + d z, lo), hi) in float32 on [N, M] depths -> [N, M, 3] (renderer_df.py:367-368)"""
    x = o.unsqueeze(-2) + d.unsqueeze(-2) * z.unsqueeze(-1)
    return torch.min(torch.max(x, aabb[:3]), aabb[3:])


# ------------------------------------------------------------------------------------------------------------------ the oracle
def restated(p, o, d, light, ratio, bg, u_coarse=None, u_fine=None, training=False, T=64):
    """run(shading='lambertian') (renderer_df.py:404-456, network_grid.py:129-153) on the CPU oracle: the albedo render's sorted
    ray, the finite-difference normals composed as point_attrs_common.oracle_attrs composes them, torch float32 for the rest."""
    with torch.no_grad():
        aux = ngp_ref.render_run(p, o, d, bound=BOUND, num_steps=T, upsample_steps=T, u_coarse=u_coarse, u_fine=u_fine,
                                 bg_color=float(bg), training=training, return_aux=True)
        N, M = aux["z_sorted"].shape
        aabb = p["aabb_train"] if training else p["aabb_infer"]
        x = sorted_points(o, d, aux["z_sorted"], aabb).reshape(-1, 3).contiguous()
        ref = pc.oracle_attrs(p, x, EPS)
        normal = torch.from_numpy(pc.np_normal(ref["grad"].numpy()))
        lam = ratio + (1 - ratio) * (normal @ -light).clamp(min=0)
        color = (aux["rgb_sorted"].reshape(-1, 3) * lam.unsqueeze(-1)).view(N, M, 3)
        w = aux["weights"]
        dirs = d.view(-1, 1, 3).expand(N, M, 3)
        cosd = (normal.view(N, M, 3) * dirs).sum(-1).clamp(min=0)
        image = torch.sum(w.unsqueeze(-1) * color, dim=-2) + (1 - aux["weights_sum"]).unsqueeze(-1) * bg
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.linalg.norm(pc.grad_bound(ref, EPS), axis=1) / np.linalg.norm(ref["grad"].double().numpy(), axis=1)
        r[np.isnan(r)] = np.inf
    return dict(aux=aux, x=x, ref=ref, normal=normal.view(N, M, 3), color=color, weights=w, image=image, image_albedo=aux["image"],
                depth=aux["depth"], weights_sum=aux["weights_sum"], loss_orient=(w * cosd ** 2).mean(),
                normal_image=torch.sum(w.unsqueeze(-1) * normal.view(N, M, 3), dim=-2), cosd=cosd,
                r=r.reshape(N, M), dnorm=d.double().norm(dim=-1).numpy())


def delta(rs):
    """per sample: how far the density tolerances let the unit normal move -- 2 r + 1e-6 (test_point_attrs_cpu.py), at most 2"""
    return np.minimum(2.0, 2.0 * rs["r"] + 1e-6)


def image_bound(rs, ratio):
    """[N]: 2e-5 + (1 - ratio) sum_i w_i delta_i (albedo <= 1, |l| = 1: the lambertian term moves by at most delta)"""
    w = rs["weights"].double().numpy()
    return 2e-5 + (1.0 - ratio) * (w * delta(rs)).sum(axis=1)


def orient_bound(rs, golden_value):
    """c = max(n . d, 0) moves by at most |d| delta, so c^2 by at most 2 c |d| delta + |d|^2 delta^2; mean over all samples"""
    w, c, dl = rs["weights"].double().numpy(), rs["cosd"].double().numpy(), delta(rs)
    dn = rs["dnorm"][:, None]
    return float((w * (2 * c * dn * dl + dn * dn * dl * dl)).mean()) + 1e-5 * float(golden_value)


# ----------------------------------------------------------------------------------------- numpy float32 restatements (bit level)
def np_points(o, d, z, aabb):
    """ngp_point: min(max(o + d * z, lo), hi), one rounding per operation; o, d [N,3], z [N,M] -> [N,M,3]"""
    o, d, z, aabb = (np.asarray(t, dtype=F32) for t in (o, d, z, aabb))
    with np.errstate(all="ignore"):
        v = o[:, None, :] + d[:, None, :] * z[:, :, None]
        return np.fmin(np.fmax(v, aabb[:3]), aabb[3:]).astype(F32)


def np_shade(albedo, normal, light, ratio):
    """albedo * (ratio + (1 - ratio) * max((n0 * -l0 + n1 * -l1) + n2 * -l2, 0)) in float32; albedo, normal [..., 3]"""
    a, n, l = (np.asarray(t, dtype=F32) for t in (albedo, normal, light))
    ratio = F32(ratio)
    with np.errstate(all="ignore"):
        dot = (n[..., 0] * -l[0] + n[..., 1] * -l[1]) + n[..., 2] * -l[2]
        lit = np.where(np.isnan(dot), dot, np.maximum(dot, F32(0)))
        lam = ratio + (F32(1) - ratio) * lit
        return (a * lam[..., None]).astype(F32)


def np_composite(z, sigma, color, normal, d, near, far, T, bg):
    """Front-to-back float32 loop over sorted rays (renderer_df.py:404-456): transmittance as a running product in double (torch's
    CPU cumprod), every sum in float32 in sample order.  -> image [N,3], depth, weights_sum, normal_image [N,3], orient [N]"""
    z, sigma, color, normal, d, near, far = (np.asarray(t, dtype=F32) for t in (z, sigma, color, normal, d, near, far))
    N, M = z.shape
    image, nimg = np.zeros((N, 3), F32), np.zeros((N, 3), F32)
    depth, ws, orient = np.zeros(N, F32), np.zeros(N, F32), np.zeros(N, F32)
    with np.errstate(all="ignore"):
        for n in range(N):
            span = far[n] - near[n]
            sample_dist = span / F32(T)
            tr = 1.0
            for m in range(M):
                dl = z[n, m + 1] - z[n, m] if m + 1 < M else sample_dist
                alpha = F32(1) - np.exp(-dl * sigma[n, m], dtype=F32)
                w = F32(alpha * F32(tr))
                tr *= float(F32(F32(1) - alpha) + F32(1e-15))
                oz = (z[n, m] - near[n]) / span
                oz = oz if np.isnan(oz) else min(max(oz, F32(0)), F32(1))
                nd = (normal[n, m, 0] * d[n, 0] + normal[n, m, 1] * d[n, 1]) + normal[n, m, 2] * d[n, 2]
                nd = nd if np.isnan(nd) else max(nd, F32(0))
                ws[n] += w
                depth[n] += w * oz
                image[n] += w * color[n, m]
                nimg[n] += w * normal[n, m]
                orient[n] += w * (nd * nd)
            image[n] += (F32(1) - ws[n]) * F32(bg)
    return image, depth, ws, nimg, orient


# ---------------------------------------------------------------------------------------------------------------- host emulation
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_SO = os.path.join(_HERE, "_build", "libshade_emu.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_handle = None


def emu_available():
    return os.path.exists(CLANG)


def _emu():
    global _handle
    if _handle is None:
        csrc = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
        deps = [os.path.join(_HERE, f) for f in ("shade_emu.cpp", "ngp_host.cpp", "ngp_emu_common.h", "hip_emu.h")] + \
               [os.path.join(csrc, f) for f in ("ngp_shade.h", "ngp_point_attrs.h", "ngp_composite_wave.h", "ngp_device.h", "sf_dev.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call([CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + _HERE, "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-Wno-source-uses-openmp", "-ffp-contract=off", deps[0], "-o", _SO,
                                   "-lpthread"])
        _handle = C.CDLL(_SO)
        for name in ("emu_shade", "emu_composite_sorted", "emu_composite_wave"):
            getattr(_handle, name).restype = None
    return _handle


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _nan(*s):
    return torch.full(s, float("nan"), dtype=torch.float32)


def emu_shade(params, o, d, aabb, z_s, albedo_s, light, ratio, eps=EPS, blocks=2, xyz=True):
    """k_ngp_shade on CPU fibers over `blocks` workgroups of 256 threads; outputs pre-filled with NaN"""
    N, M = z_s.shape
    out = dict(normal_s=_nan(N, M, 3), rgb_shaded_s=_nan(N, M, 3), xyz_s=_nan(N, M, 3) if xyz else None)
    offs = params["encoder.offsets"].contiguous()
    w = [params[f"sigma_net.net.{i}.{k}"].contiguous() for i in range(3) for k in ("weight", "bias")]
    keep = [t.contiguous().float() for t in (o, d, aabb, z_s, albedo_s, light)]
    _emu().emu_shade(_p(params["encoder.embeddings"]), _p(offs), C.c_uint32(offs.numel() - 1), C.c_float(log2_scale()), C.c_uint32(16),
                     C.c_uint32(1), *[_p(t) for t in w], C.c_float(BOUND), *[_p(t) for t in keep], C.c_uint32(N), C.c_uint32(M // 2),
                     C.c_float(ratio), C.c_float(eps), C.c_uint32(blocks), _p(out["normal_s"]), _p(out["rgb_shaded_s"]),
                     _p(out["xyz_s"]))
    return out


def emu_composite_sorted(z_s, sig_s, col_s, nrm_s, d, nears, fars, bg, normal_image=True, orient=True):
    """k_ngp_composite_sorted_wave on CPU fibers; outputs pre-filled with NaN; None for skipped ones"""
    N, M = z_s.shape
    out = dict(image=_nan(N, 3), depth=_nan(N), weights_sum=_nan(N), normal_image=_nan(N, 3) if normal_image else None,
               orient=_nan(N) if orient else None)
    keep = [t.contiguous().float() for t in (z_s, sig_s, col_s, nrm_s, d, nears, fars)]
    _emu().emu_composite_sorted(*[_p(t) for t in keep], C.c_uint32(N), C.c_uint32(M // 2), C.c_float(bg),
                                *[_p(out[k]) for k in ("image", "depth", "weights_sum", "normal_image", "orient")])
    return out


def emu_composite_wave(z_s, sig_s, rgb_s, nears, fars, bg):
    """k_ngp_composite_wave (the albedo render's kernel) on CPU fibers, fed the SORTED ray as coarse = first half, fine = second
    half: its stable rank sort is then the identity, and it composites the same sorted ray"""
    N, M = z_s.shape
    T = M // 2
    halves = [t.contiguous() for s in (z_s, sig_s, rgb_s) for t in (s[:, :T], s[:, T:])]
    z_c, z_f, s_c, s_f, r_c, r_f = halves
    out = dict(z_s=_nan(N, M), sig_s=_nan(N, M), rgb_s=_nan(N, M, 3), image=_nan(N, 3), depth=_nan(N), weights_sum=_nan(N))
    keep = [nears.contiguous().float(), fars.contiguous().float()]
    _emu().emu_composite_wave(_p(z_c), _p(s_c), _p(r_c), _p(z_f), _p(s_f), _p(r_f), _p(keep[0]), _p(keep[1]), C.c_uint32(N),
                              C.c_uint32(T), C.c_float(bg), *[_p(out[k]) for k in ("z_s", "sig_s", "rgb_s", "image", "depth", "weights_sum")])
    return out

"""Shared pieces of the point-attribute tests (sf_ngp_point_attrs; sparsefusion_amd/csrc/ngp_point_attrs.h): the point sets, the
oracle's finite-difference gradient composed as the reference composes it, the bounds the density tolerances imply for it, the
numpy float32 restatement of the gradient / normal formulas, and the ctypes harness of tests/hostemu/point_attrs_emu.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

from ngp_common import BOUND, log2_scale
from oracle import ngp_ref

EPSILONS = (1e-2, 8 / 127)
SIGMA_RTOL, SIGMA_ATOL, ALBEDO_ATOL = 2e-5, 1e-7, 1e-6         # tests/test_gpu_ngp.py::test_density_matches_oracle

SPECIAL = torch.tensor([[0.0, 0.0, 0.0]] +
                       [[sx * BOUND, sy * BOUND, sz * BOUND] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)] +
                       [[5.0, 0.3, -0.2], [-4.5, 4.25, 1.0], [0.1, 0.2, 7.0]], dtype=torch.float32)      # origin, corners, outside


def points(n, seed=3):
    """n points uniform in the box, then the origin, the eight corners and three points outside the box"""
    g = torch.Generator().manual_seed(seed)
    return torch.cat([(torch.rand(n, 3, generator=g) * 2 - 1) * BOUND, SPECIAL]).contiguous()


def spliced_points(n, seed=3):
    """n points uniform in the box with the special points written over a spread of positions (first, last, block edges)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, generator=g) * 2 - 1) * BOUND
    k = SPECIAL.shape[0]
    if n >= k:
        pos = torch.unique(torch.linspace(0, n - 1, k).round().long())
        x[pos] = SPECIAL[:pos.numel()]
    else:
        x[:] = SPECIAL[:n]
    return x.contiguous()


def offset_points(x, eps, axis, sign):
    """network_grid.py:93-98: (x + [[.., +-eps, ..]]).clamp(-bound, bound), add and clamp in float32"""
    o = [0.0, 0.0, 0.0]
    o[axis] = sign * eps
    return (x + torch.tensor([o], dtype=torch.float32, device=x.device)).clamp(-BOUND, BOUND)


def oracle_attrs(p, x, eps):
    """The CPU oracle composed as network_grid.py:91-106 in float32 -> dict of sigma [P], albedo [P,3], sp / sn [P,3] (sigma at the
    six offset points), grad [P,3]"""
    with torch.no_grad():
        sigma, albedo = ngp_ref.common_forward(p, x, BOUND)
        sp = torch.stack([ngp_ref.common_forward(p, offset_points(x, eps, a, 1.0), BOUND)[0] for a in range(3)], -1)
        sn = torch.stack([ngp_ref.common_forward(p, offset_points(x, eps, a, -1.0), BOUND)[0] for a in range(3)], -1)
        grad = 0.5 * (sp - sn) / eps
    return dict(sigma=sigma, albedo=albedo, sp=sp, sn=sn, grad=grad)


def grad_bound(ref, eps):
    """Per element: what the density tolerances allow sp and sn to move, through 0.5 * (sp - sn) / eps, plus 4 ulp of the value"""
    sp, sn = (ref[k].double().numpy() for k in ("sp", "sn"))
    return ((SIGMA_RTOL * np.abs(sp) + SIGMA_ATOL) + (SIGMA_RTOL * np.abs(sn) + SIGMA_ATOL)) * 0.5 / eps + \
        4 * np.spacing(np.abs(ref["grad"].numpy())).astype(np.float64)


def np_grad(sp, sn, eps):
    """grad = 0.5f * (sp - sn) / eps in numpy float32 (one rounding per operation)"""
    with np.errstate(all="ignore"):
        return (np.float32(0.5) * (sp.astype(np.float32) - sn.astype(np.float32))) / np.float32(eps)


def np_normal(g):
    """normal = grad / sqrtf(fmaxf((gx gx + gy gy) + gz gz, 1e-20f)), NaN -> 0, in numpy float32"""
    g = g.astype(np.float32)
    with np.errstate(all="ignore"):
        ss = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        n = g / np.sqrt(np.fmax(ss, np.float32(1e-20)))[:, None]
    n[np.isnan(n)] = 0.0
    return n


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------- files
def plain_obj_bytes(v, f):
    """the formatting rule of export_obj before colours and normals existed"""
    f1 = f.astype(np.int64) + 1
    return (("v %.9g %.9g %.9g\n" * v.shape[0]) % tuple(v.astype(np.float64).ravel().tolist()) +
            ("f %d %d %d\n" * f1.shape[0]) % tuple(f1.ravel().tolist())).encode()


def parse_obj_attrs(path):
    """-> vertices, colours (or None), normals (or None), faces (0-based), normal indices of the faces (or None)"""
    v, c, n, f, fn = [], [], [], [], []
    for line in open(path).read().splitlines():
        t = line.split()
        if t[0] == "v":
            v.append([np.float32(s) for s in t[1:4]])
            if len(t) == 7:
                c.append([np.float32(s) for s in t[4:7]])
        elif t[0] == "vn":
            n.append([np.float32(s) for s in t[1:4]])
        elif t[0] == "f":
            parts = [s.split("//") for s in t[1:4]]
            f.append([int(q[0]) - 1 for q in parts])
            if len(parts[0]) == 2:
                fn.append([int(q[1]) - 1 for q in parts])
    arr = lambda a, dt: np.array(a, dtype=dt).reshape(-1, 3) if a else None      # noqa: E731
    return arr(v, np.float32), arr(c, np.float32), arr(n, np.float32), arr(f, np.int32), arr(fn, np.int32)


# ---------------------------------------------------------------------------------------------------------------- host emulation
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_SO = os.path.join(_HERE, "_build", "libpoint_attrs_emu.so")
_handle = None


def _emu():
    global _handle
    if _handle is None:
        csrc = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
        deps = [os.path.join(_HERE, "point_attrs_emu.cpp"), os.path.join(_HERE, "ngp_host.cpp"), os.path.join(_HERE, "ngp_emu_common.h"),
                os.path.join(csrc, "ngp_point_attrs.h"), os.path.join(csrc, "ngp_device.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-mfma", "-mavx2", "-fopenmp",
                                   "-Wno-unknown-pragmas", deps[0], "-o", _SO])
        _handle = C.CDLL(_SO)
        _handle.emu_point_attrs.restype = None
    return _handle


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def emu_point_attrs(params, x, eps, blocks=3, sigma=True, albedo=True, grad=True, normal=True):
    """k_ngp_point_attrs on the CPU over `blocks` workgroups of 256 threads; outputs pre-filled with NaN; None for skipped ones"""
    x = x.contiguous()
    P = x.shape[0]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32)      # noqa: E731
    out = dict(sigma=nan(P) if sigma else None, albedo=nan(P, 3) if albedo else None, grad=nan(P, 3) if grad else None,
               normal=nan(P, 3) if normal else None)
    offs = params["encoder.offsets"].contiguous()
    w = [params[f"sigma_net.net.{i}.{k}"].contiguous() for i in range(3) for k in ("weight", "bias")]
    _emu().emu_point_attrs(_p(params["encoder.embeddings"]), _p(offs), C.c_uint32(offs.numel() - 1), C.c_float(log2_scale()),
                           C.c_uint32(16), C.c_uint32(1), *[_p(t) for t in w], C.c_float(BOUND), _p(x), C.c_uint32(P),
                           C.c_float(eps), C.c_uint32(blocks), _p(out["sigma"]), _p(out["albedo"]), _p(out["grad"]),
                           _p(out["normal"]))
    return out

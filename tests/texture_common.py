"""Shared pieces of the texture-bake tests (sf_ngp_texture_bake; sparsefusion_amd/csrc/ngp_texture.h): the atlas layout, the texel
ownership, the gutter clamp and the weighted sum restated in numpy (integers and float32, one rounding per operation), the
quantisation rule, synthetic meshes, a PNG decoder, an OBJ parser and the ctypes harness of tests/hostemu/texture_emu.cpp."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import torch

from ngp_common import BOUND, log2_scale

# (F, W): the minimum cell (W = 6 G) for F = 1, 2, 3, 7, and F = 50 at W = 64 (G = 5, c = 12: four margin texels right / below)
SMALL_CASES = ((1, 6), (2, 6), (3, 12), (7, 12), (50, 64))


def layout(F, W):
    """(G, c): G = ceil(sqrt(ceil(F / 2))), c = W // G"""
    cells = (F + 1) // 2
    G = next(g for g in range(1, cells + 1) if g * g >= cells)
    return G, W // G


def owner_half(c, i, j):
    """0: the lower face of the cell owns texel (i, j); 1: the upper"""
    return np.where(i + j <= c - 2, 0, 1)


def corner_texels(F, W):
    """integer texel (x, y) of each face corner [F, 3, 2]"""
    G, c = layout(F, W)
    leg = c - 5
    out = np.zeros((F, 3, 2), dtype=np.int64)
    for f in range(F):
        q, half = f >> 1, f & 1
        row, col = q // G, q % G
        ij = [(1, 1), (1 + leg, 1), (1, 1 + leg)] if half == 0 else [(c - 2, c - 2), (c - 2 - leg, c - 2), (c - 2, c - 2 - leg)]
        for k, (i, j) in enumerate(ij):
            out[f, k] = (col * c + i, row * c + j)
    return out


def np_bake_points(verts, faces, W):
    """The texel -> (face, point) rule restated: face_id [W, W] int32 (-1: unused) and xyz [W, W, 3] float32 (0 where unused).
    Clamp rule, in the half's own cell-local index (the upper half mirrored, i -> c - 1 - i): p = clip(i - 1, 0, l),
    q = clip(j - 1, 0, l), e = max(p + q - l, 0), p -= (e + 1) // 2, q -= e // 2; u = p / l, v = q / l, w0 = (1 - u) - v and
    x = (w0 * va + u * vb) + v * vc, every operation rounded to float32."""
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    faces = np.asarray(faces).reshape(-1, 3)
    F, V = faces.shape[0], verts.shape[0]
    face_id = np.full((W, W), -1, dtype=np.int32)
    xyz = np.zeros((W, W, 3), dtype=np.float32)
    if F == 0:
        return face_id, xyz
    G, c = layout(F, W)
    leg = c - 5
    y, x = np.meshgrid(np.arange(W), np.arange(W), indexing="ij")
    col, row = x // c, y // c
    i, j = x - col * c, y - row * c
    half = owner_half(c, i, j)
    f = 2 * (row * G + col) + half
    used = (col < G) & (row < G) & (f < F)
    fs = np.where(used, f, 0)
    idx = faces[fs]                                                              # [W, W, 3]
    used &= ((idx >= 0) & (idx < V)).all(-1)
    i = np.where(half == 1, c - 1 - i, i)
    j = np.where(half == 1, c - 1 - j, j)
    p, q = np.clip(i - 1, 0, leg), np.clip(j - 1, 0, leg)
    e = np.maximum(p + q - leg, 0)
    p, q = p - (e + 1) // 2, q - e // 2
    assert (p[used] >= 0).all() and (q[used] >= 0).all() and ((p + q)[used] <= leg).all()
    f32 = np.float32
    u, v = (p.astype(f32) / f32(leg))[..., None], (q.astype(f32) / f32(leg))[..., None]
    w0 = (f32(1.0) - u) - v
    idx = np.where(used[..., None], idx, 0)
    va, vb, vc = (verts[idx[..., k]] for k in range(3))
    pts = ((w0 * va).astype(f32) + (u * vb).astype(f32)).astype(f32) + (v * vc).astype(f32)
    xyz[used] = pts.astype(f32)[used]
    face_id[used] = f[used]
    return face_id, xyz


def np_quantise(albedo):
    """(uint8)(min(max(a, 0), 1) * 255) in float32: truncation; NaN -> 0"""
    a = np.asarray(albedo, dtype=np.float32)
    a = np.where(np.isnan(a), np.float32(0.0), a)
    return (np.minimum(np.maximum(a, np.float32(0.0)), np.float32(1.0)) * np.float32(255.0)).astype(np.float32).astype(np.uint8)


def random_mesh(F, seed=11):
    """F random triangles over V = F + 2 vertices uniform in the box -> (verts [V, 3] float32, faces [F, 3] int32)"""
    rng = np.random.default_rng(seed + F)
    V = F + 2
    verts = ((rng.random((V, 3)) * 2 - 1) * BOUND).astype(np.float32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    return verts, faces


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------- files
def decode_png(raw):
    """8-bit RGB, non-interlaced PNG with filter type 0 on every row -> [H, W, 3] uint8; every chunk's CRC is checked"""
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF, kind
        chunks.append((kind, data))
        pos += 12 + n
    assert pos == len(raw) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for k, d in chunks if k == b"IDAT")), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3).copy()


def parse_obj_textured(path):
    """-> dict: mtllib, usemtl, v [V, 3] f32, vt [T, 2] f32, vn [N, 3] f32 or None, and per face the 0-based f / ft / fn [F, 3]
    (fn None without normals)"""
    out = dict(mtllib=None, usemtl=None, order=[])
    v, vt, vn, f, ft, fn = [], [], [], [], [], []
    for line in open(path).read().splitlines():
        t = line.split()
        if not out["order"] or out["order"][-1] != t[0]:
            out["order"].append(t[0])
        if t[0] in ("mtllib", "usemtl"):
            out[t[0]] = t[1]
        elif t[0] == "v":
            v.append([np.float32(s) for s in t[1:4]])
        elif t[0] == "vt":
            vt.append([np.float32(s) for s in t[1:3]])
        elif t[0] == "vn":
            vn.append([np.float32(s) for s in t[1:4]])
        elif t[0] == "f":
            parts = [s.split("/") for s in t[1:4]]
            f.append([int(q[0]) - 1 for q in parts])
            ft.append([int(q[1]) - 1 for q in parts])
            if len(parts[0]) == 3:
                fn.append([int(q[2]) - 1 for q in parts])
    arr = lambda a, dt, k: np.array(a, dtype=dt).reshape(-1, k) if a else None      # noqa: E731
    out.update(v=arr(v, np.float32, 3), vt=arr(vt, np.float32, 2), vn=arr(vn, np.float32, 3), f=arr(f, np.int64, 3),
               ft=arr(ft, np.int64, 3), fn=arr(fn, np.int64, 3))
    return out


# ---------------------------------------------------------------------------------------------------------------- host emulation
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_SO = os.path.join(_HERE, "_build", "libtexture_emu.so")
_handle = None


def _emu():
    global _handle
    if _handle is None:
        csrc = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
        deps = [os.path.join(_HERE, "texture_emu.cpp"), os.path.join(_HERE, "ngp_host.cpp"), os.path.join(_HERE, "ngp_emu_common.h"),
                os.path.join(csrc, "ngp_texture.h"), os.path.join(csrc, "ngp_device.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-mfma", "-mavx2", "-fopenmp",
                                   "-Wno-unknown-pragmas", deps[0], "-o", _SO])
        _handle = C.CDLL(_SO)
        _handle.emu_texture_bake.restype = C.c_int
        _handle.emu_atlas_make.restype = C.c_int
    return _handle


def emu_atlas_make(F, W):
    """-> (return code of the kernel's layout / argument check, G, c)"""
    G, c = C.c_uint32(0), C.c_uint32(0)
    rc = _emu().emu_atlas_make(C.c_uint32(F), C.c_uint32(W), C.byref(G), C.byref(c))
    return rc, G.value, c.value


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def emu_texture_bake(params, verts, faces, W, blocks=3, want=("rgb8", "albedo", "xyz", "face_id")):
    """k_ngp_texture_bake on the CPU over `blocks` workgroups of 256 threads.  Outputs are pre-filled with 0xFF / NaN / INT32_MIN and
    come back as numpy ([W, W, 3] or [W, W]); None for those not in `want`.  -> (return code, dict)"""
    v = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32))
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3))
    out = dict(rgb8=torch.full((W, W, 3), 255, dtype=torch.uint8) if "rgb8" in want else None,
               albedo=torch.full((W, W, 3), float("nan")) if "albedo" in want else None,
               xyz=torch.full((W, W, 3), float("nan")) if "xyz" in want else None,
               face_id=torch.full((W, W), -2 ** 31, dtype=torch.int32) if "face_id" in want else None)
    offs = params["encoder.offsets"].contiguous()
    w = [params[f"sigma_net.net.{i}.{k}"].contiguous() for i in range(3) for k in ("weight", "bias")]
    rc = _emu().emu_texture_bake(_p(params["encoder.embeddings"]), _p(offs), C.c_uint32(offs.numel() - 1), C.c_float(log2_scale()),
                                 C.c_uint32(16), C.c_uint32(1), *[_p(t) for t in w], C.c_float(BOUND), _p(v), C.c_uint32(v.shape[0]),
                                 _p(f), C.c_uint32(f.shape[0]), C.c_uint32(W), C.c_uint32(blocks), _p(out["rgb8"]), _p(out["albedo"]),
                                 _p(out["xyz"]), _p(out["face_id"]))
    return rc, {k: (t.numpy() if t is not None else None) for k, t in out.items()}

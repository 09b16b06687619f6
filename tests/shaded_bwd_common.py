"""Shared pieces of the shaded-render BACKWARD tests (sf_ngp_render_shaded_backward; sparsefusion_amd/csrc/ngp_shade_bwd.h): the closed
form of DESIGN 9.7 in float64 next to the torch.autograd graph it restates, the oracle restatement of the reference's differentiable
run(shading='lambertian') composed from ngp_ref.render_run + ngp_ref.common_forward at the six offsets, the per-element rounding
bounds of k_ngp_shade_bwd, and the ctypes harness of tests/hostemu/shade_bwd_emu.cpp."""
import ctypes as C
import os
import subprocess

import torch

import ngp_bwd_cases as nb
import shaded_common as sc
from ngp_common import BOUND, grad_leaf, log2_scale
from oracle import ngp_ref

EPS = sc.EPS
U24, TINY = nb.U24, nb.TINY
MLP_NAMES = [f"sigma_net.net.{i}.{w}" for i in range(3) for w in ("weight", "bias")]


# ------------------------------------------------------------------------------------------------ section 1 of the issue, two ways
def shade_graph(s_off, alb, w, d, light, ratio, eps):
    """The reference's graph from the six offset densities s_off [P, 6] (x+, x-, y+, y-, z+, z-) and the albedo [P, 3] to the shaded
    colour [P, 3] and the orientation term w max(n . d, 0)^2 [P] (w detached), in the dtype of its inputs.  network_grid.py:100-104,
    155-164, 188-195; utils.py:41 (safe_normalize); renderer_df.py:430."""
    g = torch.stack([0.5 * (s_off[:, 0] - s_off[:, 1]) / eps, 0.5 * (s_off[:, 2] - s_off[:, 3]) / eps,
                     0.5 * (s_off[:, 4] - s_off[:, 5]) / eps], -1)
    n = g / torch.sqrt(torch.clamp((g * g).sum(-1, keepdim=True), min=1e-20))
    n = torch.where(torch.isnan(n), torch.zeros_like(n), n)
    lam = ratio + (1 - ratio) * (n @ -light).clamp(min=0)
    col = alb * lam.unsqueeze(-1)
    orient = w.detach() * (n * d).sum(-1).clamp(min=0) ** 2
    return dict(g=g, n=n, lam=lam, col=col, orient=orient)


def shade_bwd_closed(dcol, alb, n, g, w, d, light, ratio, eps, g_orient):
    """The closed form k_ngp_shade_bwd evaluates, in the dtype of its inputs: d(albedo) [P, 3], d(n), d(g) [P, 3], d(s_e) [P, 6].
    g_orient [P]: the ray's upstream of the orientation term at every sample.  Non-finite g: d(g) = 0 (the deviation)."""
    ml = -light
    lam = ratio + (1 - ratio) * (n @ ml).clamp(min=0)
    da = dcol * lam.unsqueeze(-1)
    lit = ((n @ ml) > 0).to(dcol.dtype)
    nd = (n * d).sum(-1)
    dn = ((1 - ratio) * lit * (alb * dcol).sum(-1)).unsqueeze(-1) * ml + \
         (g_orient * w * 2 * nd.clamp(min=0) * (nd > 0).to(dcol.dtype)).unsqueeze(-1) * d
    G = (g * g).sum(-1, keepdim=True)
    length = torch.sqrt(torch.clamp(G, min=1e-20))
    dg = torch.where(G >= 1e-20, (dn - n * (n * dn).sum(-1, keepdim=True)) / length, dn / length)
    dg = torch.where(torch.isfinite(g).all(-1, keepdim=True), dg, torch.zeros_like(dg))
    k = 0.5 / eps
    ds = torch.stack([k * dg[:, 0], -k * dg[:, 0], k * dg[:, 1], -k * dg[:, 1], k * dg[:, 2], -k * dg[:, 2]], -1)
    return dict(da=da, dn=dn, dg=dg, ds=ds, lam=lam)


def shade_bwd_bound(dcol, alb, n, g, w, d, light, ratio, eps, g_orient):
    """float64 want and per-element rounding bound of k_ngp_shade_bwd's outputs from ITS fp32 inputs (u = 2^-24, first order): every
    fp32 operation rounds once, relative to the magnitude of its TERMS.  A dot product of three: 5 u sum|terms|.
      lam  = ratio + (1 - ratio) max(n . -l, 0):            d_lam = 8 u (|ratio| + |1 - ratio| sum|n_i l_i|)
      da   = dcol lam:                                       d = |dcol| d_lam + u |da|
      s_lit = (1 - ratio)(a . dcol), s_ori = (go w)(2 nd):   d_s_lit = 7 u |1 - ratio| sum|a_i dcol_i|,  d_s_ori = 8 u |go w| 2 sum|n_i d_i|
      dn_c = s_lit (-l_c) + s_ori d_c:                       d = |l_c| d_s_lit + |d_c| d_s_ori + 3 u (|s_lit l_c| + |s_ori d_c|)
      G, len: 6 u G on G (positive terms), so 4 u len on len (sqrt halves it, + its own rounding)
      q = n . dn: d_q = sum|n_i| d_dn_i + 5 u sum|n_i dn_i|;   t_c = dn_c - n_c q: d = d_dn_c + |n_c| d_q + 2 u (|dn_c| + |n_c q|)
      dg_c = t_c / len: d = d_t / len + 5 u |t_c| / len;       ds = k dg, k = 0.5 / eps: d = |k| d_dg + 2 u |ds|
    The two selects ([n . -l > 0], [n . d > 0]) are evaluated on the same fp32 n, l, d on both sides: a sample whose dot product lies
    within 5 u sum|terms| of zero is `ambiguous` and left out of the comparison of dn / dg / ds (returned mask)."""
    f = lambda t: t.double()
    dcol, alb, n, g, w, d, light, g_orient = (f(t) for t in (dcol, alb, n, g, w, d, light, g_orient))
    want = shade_bwd_closed(dcol, alb, n, g, w, d, light, ratio, eps, g_orient)
    ml = -light
    absdot = lambda a, b: (a.abs() * b.abs()).sum(-1)
    lit_dot, nd = n @ ml, (n * d).sum(-1)
    amb = (lit_dot.abs() <= 5 * U24 * absdot(n, ml.expand_as(n))) | (nd.abs() <= 5 * U24 * absdot(n, d))
    amb = amb & ((lit_dot != 0) | (nd != 0))                      # n == 0 (a flat or non-finite gradient) is exact on both sides
    d_lam = 8 * U24 * (abs(ratio) + abs(1 - ratio) * absdot(n, ml.expand_as(n)))
    b_da = dcol.abs() * d_lam.unsqueeze(-1) + U24 * want["da"].abs() + TINY
    s_lit = (1 - ratio) * (lit_dot > 0) * (alb * dcol).sum(-1)
    s_ori = g_orient * w * 2 * nd.clamp(min=0)
    d_s_lit = 7 * U24 * abs(1 - ratio) * absdot(alb, dcol) * (lit_dot > 0)
    d_s_ori = 8 * U24 * (g_orient * w).abs() * 2 * absdot(n, d) * (nd > 0)
    b_dn = ml.abs() * d_s_lit.unsqueeze(-1) + d.abs() * d_s_ori.unsqueeze(-1) + \
        3 * U24 * ((s_lit.unsqueeze(-1) * ml).abs() + (s_ori.unsqueeze(-1) * d).abs()) + TINY
    G = (g * g).sum(-1, keepdim=True)
    length = torch.sqrt(torch.clamp(G, min=1e-20))
    q = torch.where(G >= 1e-20, (n * want["dn"]).sum(-1, keepdim=True), torch.zeros_like(G))
    d_q = torch.where(G >= 1e-20, (n.abs() * b_dn).sum(-1, keepdim=True) + 5 * U24 * absdot(n, want["dn"]).unsqueeze(-1), torch.zeros_like(G))
    t = want["dn"] - n * q
    d_t = b_dn + n.abs() * d_q + 2 * U24 * (want["dn"].abs() + (n * q).abs())
    b_dg = d_t / length + 5 * U24 * t.abs() / length + TINY
    b_dg = torch.where(torch.isfinite(g).all(-1, keepdim=True), b_dg, torch.zeros_like(b_dg))
    k = 0.5 / eps
    b_ds = (k * b_dg).repeat_interleave(2, dim=-1) + 2 * U24 * want["ds"].abs() + TINY
    return dict(want=want, da_bound=b_da, dn_bound=b_dn, dg_bound=b_dg, ds_bound=b_ds, ambiguous=amb)


# ------------------------------------------------------------------------------------------------------------------ the oracle
def offset_points(x, eps=EPS, bound=BOUND):
    """[P, 3] fp32 -> [6, P, 3]: clamp(x + (+-eps) e_axis, -bound, bound) as finite_difference_normal builds them (the add and the clamp
    on all three coordinates)."""
    out = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            off = torch.zeros(1, 3, dtype=x.dtype)
            off[0, axis] = sign * eps
            out.append((x + off).clamp(-bound, bound))
    return torch.stack(out)


def restated_grad(p, o, d, light, ratio, bg, u_coarse, u_fine, g_image, g_ws, lam, training=True, T=64):
    """The reference's differentiable run(shading='lambertian') on the CPU oracle under torch autograd (fp32):
    loss = (image g_image).sum() + (weights_sum g_ws).sum() + lam loss_orient.  ngp_ref.render_run gives the sorted ray, its weights
    and the albedo with their graph; ngp_ref.common_forward at the six offset points gives the densities of the normal.
    -> the leaf parameters (with .grad), d loss / d sigma of the sorted ray, and the forward values."""
    pl = grad_leaf(p)
    aux = ngp_ref.render_run(pl, o, d, bound=BOUND, num_steps=T, upsample_steps=T, u_coarse=u_coarse, u_fine=u_fine, bg_color=float(bg),
                             training=training, return_aux=True)
    aux["sigma_sorted"].retain_grad()
    N, M = aux["z_sorted"].shape
    aabb = p["aabb_train"] if training else p["aabb_infer"]
    x = sc.sorted_points(o, d, aux["z_sorted"].detach(), aabb).reshape(-1, 3)
    s_off = torch.stack([ngp_ref.common_forward(pl, xe, BOUND)[0] for xe in offset_points(x)], -1)
    w = aux["weights"]
    dirs = d.view(-1, 1, 3).expand(N, M, 3).reshape(-1, 3)
    sh = shade_graph(s_off, aux["rgb_sorted"].reshape(-1, 3), w.reshape(-1), dirs, light, ratio, EPS)
    image = torch.sum(w.unsqueeze(-1) * sh["col"].view(N, M, 3), dim=-2) + (1 - aux["weights_sum"]).unsqueeze(-1) * bg
    orient = sh["orient"].view(N, M).sum(-1)
    loss_orient = sh["orient"].mean()
    loss = (image * g_image).sum() + (aux["weights_sum"] * g_ws).sum() + lam * loss_orient
    loss.backward()
    return dict(params=pl, aux=aux, image=image.detach(), weights_sum=aux["weights_sum"].detach(), orient=orient.detach(),
                loss_orient=loss_orient.detach(), dsigma=aux["sigma_sorted"].grad, grad_s=sh["g"].detach().view(N, M, 3),
                normal_s=sh["n"].detach().view(N, M, 3), col_s=sh["col"].detach().view(N, M, 3), x=x)


def table_summary(ge, offsets):
    """norm and per-level absolute sums of a table gradient (what tests/golden/ngp_render.pt keeps)"""
    return ge.norm(), torch.stack([ge[offsets[l]:offsets[l + 1]].abs().sum() for l in range(16)])


# ---------------------------------------------------------------------------------------------------------------- host emulation
_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_SO = os.path.join(_HERE, "_build", "libshade_bwd_emu.so")
_handle = None


def emu_available():
    return sc.emu_available()


def _emu():
    global _handle
    if _handle is None:
        csrc = os.path.join(_HERE, "..", "..", "sparsefusion_amd", "csrc")
        deps = [os.path.join(_HERE, f) for f in ("shade_bwd_emu.cpp", "ngp_host.cpp", "ngp_emu_common.h", "hip_emu.h")] + \
               [os.path.join(csrc, f) for f in ("ngp_shade_bwd.h", "ngp_point_attrs.h", "ngp_bwd_mfma.h", "ngp_scatter_bin.h",
                                                "ngp_bwd_plan.h", "ngp_device.h", "sf_dev.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in deps):
            os.makedirs(os.path.dirname(_SO), exist_ok=True)
            subprocess.check_call([sc.CLANG, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + _HERE, "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-Wno-source-uses-openmp", "-ffp-contract=off", deps[0], "-o", _SO,
                                   "-lpthread"])
        _handle = C.CDLL(_SO)
        for name in ("emu_shade_bwd", "emu_offset_points", "emu_field_bwd_off", "emu_offset_features", "emu_scatter_ref64"):
            getattr(_handle, name).restype = None
        _handle.emu_bin_scatter_off.restype = C.c_int
    return _handle


_p = sc._p


def _field_args(params):
    offs = params["encoder.offsets"].contiguous()
    w = [params[f"sigma_net.net.{i}.{k}"].contiguous() for i in range(3) for k in ("weight", "bias")]
    return offs, w


def emu_shade_bwd(dcol, alb, nrm, grad, w, d, light, ratio, eps, g_orient, blocks=2):
    """k_ngp_shade_bwd on CPU fibers: [N, M, ...] fp32 tensors -> d(albedo) [N, M, 3], ds_off [6, N, M]; outputs pre-filled with NaN"""
    N, M = w.shape
    keep = [t.contiguous().float() for t in (dcol, alb, nrm, grad, w, d, light)]
    go = g_orient.contiguous().float() if g_orient is not None else None
    da, ds = sc._nan(N, M, 3), sc._nan(6, N, M)
    _emu().emu_shade_bwd(*[_p(t) for t in keep], _p(go), C.c_uint32(N), C.c_uint32(M // 2), C.c_float(ratio), C.c_float(eps),
                         C.c_uint32(blocks), _p(da), _p(ds))
    return da, ds


def emu_offset_points(o, d, aabb, z_s, e, eps=EPS, bound=BOUND):
    """ngp_point + ngp_offset_point (the backward kernels' point) for every sorted sample -> [N, M, 3]"""
    N, M = z_s.shape
    keep = [t.contiguous().float() for t in (o, d, aabb, z_s)]
    out = sc._nan(N, M, 3)
    _emu().emu_offset_points(*[_p(t) for t in keep], C.c_uint32(N), C.c_uint32(M), C.c_uint32(e), C.c_float(eps), C.c_float(bound), _p(out))
    return out


def emu_field_bwd_off(params, o, d, aabb, z_s, ds_e, e, grid, thr, eps=EPS):
    """k_ngp_field_bwd_mfma_t<1> on CPU fibers for offset e: the six MLP gradients, d(feat) [P, 32], and the features / points / inside
    flags ngp_encode gives the offset points (what the kernel's re-gather computes)"""
    N, M = z_s.shape
    P = N * M
    offs, w = _field_args(params)
    keep = [t.contiguous().float() for t in (o, d, aabb, z_s, ds_e)]
    grads = [torch.zeros_like(t) for t in w]
    dfeat = torch.zeros(16, P, 2)
    feat, xyz, inside = torch.zeros(P, 32), torch.zeros(P, 3), torch.zeros(P)
    _emu().emu_field_bwd_off(_p(params["encoder.embeddings"]), _p(offs), C.c_uint32(offs.numel() - 1), C.c_float(log2_scale()), C.c_uint32(16),
                             C.c_uint32(1), *[_p(t) for t in w], C.c_float(BOUND), *[_p(t) for t in keep], C.c_uint32(P), C.c_uint32(M),
                             C.c_uint32(grid), C.c_float(thr), C.c_uint32(e), C.c_float(eps), *[_p(t) for t in grads], _p(dfeat), _p(feat),
                             _p(xyz), _p(inside))
    return dict(grads=grads, dfeat=dfeat.permute(1, 0, 2).reshape(P, 32), feat=feat, x=xyz, inside=inside > 0, W=w)


def emu_bin_scatter_off(params, o, d, aabb, z_s, dfeat, e, first_level, cap, chunks, grid, use_ref, eps=EPS):
    """k_ngp_bin_t<1> + k_ngp_bin_reduce at offset e (use_ref: ngp_scatter on the same offset points, serial) -> table gradient"""
    N, M = z_s.shape
    offs, _ = _field_args(params)
    keep = [t.contiguous().float() for t in (o, d, aabb, z_s)]
    df = dfeat.view(N * M, 16, 2).permute(1, 0, 2).contiguous()
    gt = torch.zeros_like(params["encoder.embeddings"])
    rc = _emu().emu_bin_scatter_off(_p(offs), C.c_uint32(offs.numel() - 1), C.c_float(log2_scale()), C.c_uint32(16), C.c_uint32(1), C.c_float(BOUND),
                                    *[_p(t) for t in keep], _p(df), C.c_uint32(N), C.c_uint32(M), C.c_uint32(first_level), C.c_uint32(cap),
                                    C.c_uint32(chunks), C.c_uint32(grid), C.c_int(use_ref), C.c_uint32(e), C.c_float(eps), _p(gt))
    assert rc == 0, rc
    return gt


def emu_offset_features(params, o, d, aabb, z_s, e, eps=EPS):
    """ngp_encode at offset point e of every sorted sample, on the CPU (no kernel): features [P, 32], points [P, 3], inside [P]"""
    N, M = z_s.shape
    P = N * M
    offs, _ = _field_args(params)
    keep = [t.contiguous().float() for t in (o, d, aabb, z_s)]
    feat, xyz, inside = torch.zeros(P, 32), torch.zeros(P, 3), torch.zeros(P)
    _emu().emu_offset_features(_p(params["encoder.embeddings"]), _p(offs), C.c_uint32(offs.numel() - 1), C.c_float(log2_scale()), C.c_uint32(16),
                               C.c_uint32(1), C.c_float(BOUND), *[_p(t) for t in keep], C.c_uint32(P), C.c_uint32(M), C.c_uint32(e), C.c_float(eps),
                               _p(feat), _p(xyz), _p(inside))
    return feat, xyz, inside > 0


def scatter_ref64(params, o, d, aabb, z_s, dfeat, level, e, eps=EPS, gridtype=1):
    """Float64 table gradient of one level from d(feat) [P, 32] at offset e -> want, sum_abs, count, each [rows of the level, 2].
    Only params["encoder.offsets"] is read (any table size); gridtype 1 = tiled (the teacher field), 0 = hash."""
    N, M = z_s.shape
    P = N * M
    offs = params["encoder.offsets"].to(torch.int32).contiguous()
    rows = int(offs[level + 1] - offs[level])
    keep = [t.contiguous().float() for t in (o, d, aabb, z_s)]
    df = dfeat.view(P, 16, 2).permute(1, 0, 2).contiguous().float()
    want, sum_abs, count = (torch.zeros(rows, 2, dtype=torch.float64) for _ in range(3))
    _emu().emu_scatter_ref64(_p(offs), C.c_uint32(offs.numel() - 1), C.c_float(log2_scale()), C.c_uint32(16), C.c_uint32(gridtype), C.c_float(BOUND),
                             *[_p(t) for t in keep], _p(df), C.c_uint32(P), C.c_uint32(M), C.c_uint32(level), C.c_uint32(e), C.c_float(eps),
                             _p(want), _p(sum_abs), _p(count))
    return want, sum_abs, count


def scatter_bound(want, sum_abs, count, merged, fp32_addends=False):
    """Per element: every contribution w df is one fp32 product (u), on a z-dropped level behind one fp32 sum of two corner weights (u), and
    in a pair entry of the binned scatter the smaller corner's is rebuilt as a * (wl / wh): two more roundings (2 u) -- 4 u sum|terms|.
    `merged` (the levels of k_ngp_scatter): equal rows of up to 32 consecutive samples of a ray are first summed in an fp32 register, a chain
    of at most 32 additions: + 32 u sum|terms|.  Each addend is rounded once to 2^-44 fixed point (2^-45 each); one conversion to fp32.
    `fp32_addends` (a threshold low enough that addends take sf_grad_add's fp32 atomic): the chain term of tests/ngp_bwd_cases.py -- k
    addends in any order cost k u sum|addend|, with k <= count and the sum <= sum|terms| -- and the final rounding is 3 u |want|."""
    b = (4.0 + (32.0 if merged else 0.0)) * U24 * sum_abs + count * 2.0 ** -45 + TINY
    if fp32_addends:
        b = b + count * U24 * sum_abs
    return b + (3.0 if fp32_addends else 1.0) * U24 * (want.abs() + b)


# ------------------------------------------------------------------------------------------------------------------- descent
DESCENT = dict(n_side=8, view=3, T=16, seed=77, ratio=0.1, bg=1.0, target=0.5, lam=10.0, lr=1e-3, steps=10)
# oracle_descent's own first and last loss on the teacher field with these settings (tests/test_shaded_bwd_cpu.py pins them): the margin
# the GPU descent test halves
DESCENT_ORACLE = (0.24135, 0.20555)


def descent_problem():
    """64 rays (one misses the box), fixed draws and light of the descent test"""
    c = DESCENT
    o, d = ngp_ref.circle_rays(c["n_side"], view=c["view"])
    o, d = o.clone(), d.clone()
    o[5] = torch.tensor([20.0, 20.0, 20.0]); d[5] = torch.tensor([1.0, 0.0, 0.0])
    g = torch.Generator().manual_seed(c["seed"])
    uc, uf = torch.rand(o.shape[0], c["T"], generator=g), torch.rand(o.shape[0], c["T"], generator=g)
    light = torch.tensor([0.3, -0.5, 0.81])
    return o, d, uc, uf, light / light.norm()


def oracle_descent(p):
    """The CPU oracle's own run of the descent test: torch.optim.Adam on L1(image, target) + lam loss_orient -> the loss per step (the
    last entry is the loss after the last update)"""
    c = DESCENT
    o, d, uc, uf, light = descent_problem()
    pl = grad_leaf(p)
    leaves = [pl["encoder.embeddings"]] + [pl[k] for k in MLP_NAMES]
    opt = torch.optim.Adam(leaves, lr=c["lr"])
    losses = []
    for step in range(c["steps"] + 1):
        aux = ngp_ref.render_run(pl, o, d, bound=BOUND, num_steps=c["T"], upsample_steps=c["T"], u_coarse=uc, u_fine=uf, bg_color=c["bg"],
                                 training=True, return_aux=True)
        N, M = aux["z_sorted"].shape
        x = sc.sorted_points(o, d, aux["z_sorted"].detach(), p["aabb_train"]).reshape(-1, 3)
        s_off = torch.stack([ngp_ref.common_forward(pl, xe, BOUND)[0] for xe in offset_points(x)], -1)
        w = aux["weights"]
        sh = shade_graph(s_off, aux["rgb_sorted"].reshape(-1, 3), w.reshape(-1), d.view(-1, 1, 3).expand(N, M, 3).reshape(-1, 3), light,
                         c["ratio"], EPS)
        image = torch.sum(w.unsqueeze(-1) * sh["col"].view(N, M, 3), dim=-2) + (1 - aux["weights_sum"]).unsqueeze(-1) * c["bg"]
        loss = (image - c["target"]).abs().mean() + c["lam"] * sh["orient"].mean()
        losses.append(float(loss.detach()))
        if step == c["steps"]:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    return losses

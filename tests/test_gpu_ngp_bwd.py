"""Per-element float64 parity of the fused NGP render backward on the GPU (sf_ngp_render_backward: k_ngp_composite_bwd_wave, then
k_ngp_field_bwd_mfma), against the references and derived bounds of tests/ngp_bwd_cases.py.  The C ABI is driven directly -- forward with a
field cache, then the backward -- so that T is free; d(sigma), d(rgb) and d(feat) are read from the workspace ([0, M), [M, 4M) and [4M, 36M)
level-major, M = 2 N T).  Stage B is checked on the d(sigma) / d(rgb) the GPU's own stage A produced, so each stage stands alone.  The table
gradient of pass 0 is checked per element on small shapes at the end of this file, one level of each scatter kernel (csrc/ngp_scatter.h,
ngp_scatter_bin.h) on the d(feat) the GPU's own stage B produced; the renders of tests/test_gpu_ngp.py hold it to a norm.
Margins: profiles/ngp_bwd_parity_margins.log."""
import ctypes as C
import functools

import pytest
import torch

import ngp_bwd_cases as nb
import shaded_bwd_common as sb
from ngp_common import log2_scale, params_from_cfg
from oracle import ngp_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")


@functools.lru_cache(maxsize=None)
def _golden(golden_dir):
    g = torch.load(f"{golden_dir}/ngp_render.pt")["teacher"]
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    p = params_from_cfg(g["cfg"])
    net = NeRFNetwork(get_default_torch_ngp_opt())
    net.load_state_dict({k: p[k] for k in net.state_dict().keys()})
    return g, p, net.to(DEV)


def _forward(net, p, o, d, T, uc, uf):
    """sf_ngp_render_forward with a field cache: the sorted ray and the fp32 features of every sorted sample (cache rows through perm)."""
    from sparsefusion_amd import _lib
    from sparsefusion_amd.nerf.renderer import _FieldHandle
    N = o.shape[0]
    h = _FieldHandle(net)
    params = [t.detach().contiguous() for t in net._field_params()]
    f = h.struct(params)
    lib = _lib.lib()
    f32 = dict(dtype=torch.float32, device=DEV)
    od, dd, aabb = o.to(DEV).contiguous(), d.to(DEV).contiguous(), p["aabb_train"].to(DEV).contiguous()
    lin = torch.linspace(0.0, 1.0, T).to(DEV)
    ucd, ufd = uc.to(DEV).contiguous(), uf.to(DEV).contiguous()
    nears, fars = torch.empty(N, **f32), torch.empty(N, **f32)
    z_s, sig_s, rgb_s = torch.empty(N, 2 * T, **f32), torch.empty(N, 2 * T, **f32), torch.empty(N, 2 * T, 3, **f32)
    image, depth, ws = torch.empty(N, 3, **f32), torch.empty(N, **f32), torch.empty(N, **f32)
    wb = lib.sf_ngp_render_forward_workspace_bytes(N, T)
    work = torch.empty(wb // 4, **f32)
    cache = torch.empty(lib.sf_ngp_render_cache_bytes(N, T) // 4, **f32)
    _lib.check(lib.sf_ngp_render_forward(C.byref(f), _lib.ptr(od), _lib.ptr(dd), _lib.ptr(aabb), N, T, 0.1, _lib.ptr(lin), _lib.ptr(ucd),
                                         _lib.ptr(ufd), T, 0.0, _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(z_s), _lib.ptr(sig_s), _lib.ptr(rgb_s),
                                         _lib.ptr(image), _lib.ptr(depth), _lib.ptr(ws), _lib.ptr(cache), _lib.ptr(work), wb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    NT = N * T
    perm = cache[2 * NT * 32:2 * NT * 32 + 2 * NT].view(torch.int32).view(N, 2 * T).long()
    rows = torch.cat([cache[:NT * 32].view(N, T, 32), cache[NT * 32:2 * NT * 32].view(N, T, 32)], 1)
    feat = torch.gather(rows, 1, perm[..., None].expand(-1, -1, 32)).reshape(N * 2 * T, 32).cpu()
    x, inside = nb.sample_points(o, d, z_s.cpu(), p["aabb_train"], net.bound)
    return dict(N=N, T=T, o=od, d=dd, aabb=aabb, nears=nears, fars=fars, z_s=z_s, sig_s=sig_s, rgb_s=rgb_s, cache=cache, feat=feat,
                x=x.reshape(-1, 3), inside=inside.reshape(-1), params=params, handle=h,
                W=[t.cpu() for t in params[1:]])


def _backward(fwd, gi, gw, use_cache=True, sigma=None, rays_per_row=0):
    """sf_ngp_render_backward on a forward's sorted ray -> the six MLP gradients, the table gradient, d(sigma) [N, 2T], d(rgb) [N, 2T, 3],
    d(feat) [M, 32] (CPU)."""
    from sparsefusion_amd import _lib
    N, T = fwd["N"], fwd["T"]
    M = N * 2 * T
    grads = [torch.zeros_like(t) for t in fwd["params"]]
    gs = _lib.SfNgpFieldGrad()
    (gs.g_embeddings, gs.g_w0, gs.g_b0, gs.g_w1, gs.g_b1, gs.g_w2, gs.g_b2) = (t.data_ptr() for t in grads)
    f = fwd["handle"].struct(fwd["params"])
    lib = _lib.lib()
    wb = lib.sf_ngp_render_workspace_bytes(N, T)
    work = torch.empty(wb // 4, device=DEV)
    sig = fwd["sig_s"] if sigma is None else sigma.to(DEV).contiguous()
    gid, gwd = gi.to(DEV).contiguous(), gw.to(DEV).contiguous()
    _lib.check(lib.sf_ngp_render_backward(C.byref(f), C.byref(gs), _lib.ptr(fwd["o"]), _lib.ptr(fwd["d"]), _lib.ptr(fwd["aabb"]), N, T,
                                          _lib.ptr(fwd["nears"]), _lib.ptr(fwd["fars"]), _lib.ptr(fwd["z_s"]), _lib.ptr(sig), _lib.ptr(fwd["rgb_s"]),
                                          0.0, _lib.ptr(gid), _lib.ptr(gwd), rays_per_row, _lib.ptr(fwd["cache"]) if use_cache else None, _lib.ptr(work), wb,
                                          _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dict(grads=[t.cpu() for t in grads[1:]], table=grads[0].cpu(), dsig=work[:M].view(N, 2 * T).cpu(), drgb=work[M:4 * M].view(N, 2 * T, 3).cpu(),
                dfeat=work[4 * M:36 * M].view(16, M, 2).permute(1, 0, 2).reshape(M, 32).cpu(), sigma=sig.cpu())


def _check(name, fwd, bwd, gi, gw, geo=None, fw=None):
    """Stage A, stage B and the six MLP gradients of one backward, per element; returns what the callers report or assert further."""
    N, T = fwd["N"], fwd["T"]
    geo = nb.bwd_geometry(N, T) if geo is None else geo
    a = nb.composite_bwd_ref64(fwd["z_s"].cpu(), bwd["sigma"], fwd["rgb_s"].cpu(), fwd["nears"].cpu(), fwd["fars"].cpu(), T, 0.0, gi, gw)
    nb.check_elements(f"{name} A dsig", bwd["dsig"], a["dsig"], a["dsig_bound"], mask=a["mask"][:, None].expand(-1, 2 * T))
    nb.check_elements(f"{name} A drgb", bwd["drgb"], a["drgb"], a["drgb_bound"], mask=a["mask"][:, None, None].expand(-1, 2 * T, 3))
    if fw is None:
        fw = nb.field_forward64(fwd["feat"], fwd["W"], fwd["x"], bwd["dsig"].reshape(-1), bwd["drgb"].reshape(-1, 3))
    k, n_amb, n_left, P = nb.ambiguity(fw)
    assert n_amb <= nb.AMBIGUOUS_CAP * P and n_left <= nb.LEFT_OUT_CAP * P, (name, n_amb, n_left, P)        # conditions on the reference alone
    bk = nb.field_backward_check(f"{name} B", fw, fwd["W"], fwd["inside"], bwd["dfeat"])
    ref = nb.weight_grads_ref64(fw, bk, geo)
    flips = nb.flip_effect(fw, bk)
    print(f"counts {name}: points {P} ambiguous {n_amb} left out {n_left} inferred masks differing from the float64 sign {bk['inferred']} "
          f"(they move dw0 / db0 / dw1 / db1 by {flips['w0']:.1e} / {flips['b0']:.1e} / {flips['w1']:.1e} / {flips['b1']:.1e} rel L2)")
    for key, got in zip(KEYS, bwd["grads"]):
        r = ref[key]
        nb.check_elements(f"{name} d{key}", got, r["want"], r["bound"])
        nz = r["sum_abs"] > 0
        print(f"bound {name} d{key}: median bound / (u sum|t|) {float((r['bound'][nz] / (nb.U24 * r['sum_abs'][nz])).median()):.1f} "
              f"largest bound / norm {float(r['bound'].max() / r['want'].norm()):.2e} elements with fp32 addends {int((r['sure_fp32'] > 0).sum())} "
              f"largest wave sum {r['max_wave_sum']:.3g} thr {geo['thr']:g}")
    return dict(a=a, fw=fw, bk=bk, ref=ref, geo=geo)


def _upstream(N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 3, generator=g), torch.randn(N, generator=g)


@functools.lru_cache(maxsize=None)
def _circle_forward(golden_dir, n_side, n_rays, T, view, seed):
    g, p, net = _golden(golden_dir)
    o, d = ngp_ref.circle_rays(n_side, view=view)
    o, d = o[:n_rays].contiguous(), d[:n_rays].contiguous()
    gen = torch.Generator().manual_seed(seed)
    return _forward(net, p, o, d, T, torch.rand(n_rays, T, generator=gen), torch.rand(n_rays, T, generator=gen))


@functools.lru_cache(maxsize=None)
def _golden_forward(golden_dir):
    g, p, net = _golden(golden_dir)
    return _forward(net, p, g["rays_o"], g["rays_d"], 64, g["u_coarse"], g["u_fine"])


def test_ragged_one_chunk(golden_dir):
    """37 rays x T = 11: one chunk of 814 points, 26 trips on 7 workgroups, the last trip ragged (14 points: the scalar d(feat) stores)."""
    fwd = _circle_forward(golden_dir, 7, 37, 11, 2, 11)
    gi, gw = _upstream(37, 1)
    r = _check("ragged 37x11", fwd, _backward(fwd, gi, gw), gi, gw)
    assert r["geo"]["chunks"] == nb.CASES["ragged"]["chunks"]


def test_golden_rays(golden_dir):
    """The 256 golden rays x 64 (a miss ray among them): exactly 1024 trips, so 256 workgroups of one trip per wave -- cache and re-gather run.
    This is the per-element statement behind test_render_backward_isolated_tight's 1e-2 norm bound."""
    g, p, net = _golden(golden_dir)
    fwd = _golden_forward(golden_dir)
    assert int((fwd["nears"] >= fwd["fars"]).sum()) >= 1
    gi, gw = g["g_image"], g["g_ws"]
    r = _check("golden 256x64 cache", fwd, _backward(fwd, gi, gw), gi, gw)
    assert r["geo"]["chunks"] == nb.CASES["golden"]["chunks"]
    _check("golden 256x64 regather", fwd, _backward(fwd, gi, gw, use_cache=False), gi, gw)


@pytest.mark.parametrize("use_cache", [True, False], ids=["cache", "regather"])
def test_two_chunks(golden_dir, use_cache):
    """64 x 64 circle rays x T = 16: two chunks of 2048 rays (p_off = 65536 in the second), 2048 trips per chunk on 256 workgroups: two trips per
    wave.  The re-gather run (field_cache = NULL) is held to the same reference and bounds: its loop is the fmaf chain of the forward's encode."""
    fwd = _circle_forward(golden_dir, 64, 4096, 16, 3, 12)
    gi, gw = _upstream(4096, 2)
    r = _check(f"two chunks 4096x16 {'cache' if use_cache else 'regather'}", fwd, _backward(fwd, gi, gw, use_cache=use_cache), gi, gw)
    assert r["geo"]["chunks"] == nb.CASES["two_chunks"]["chunks"] and r["geo"]["thr"] == 128.0
    assert all(int(v["maybe_fp32"].sum()) == 0 for v in r["ref"].values())            # every wave sum below thr_mlp: the fixed-point path alone


def test_unequal_chunks(golden_dir):
    """100 x 100 circle rays x T = 8: chunks of 8192 and 1808 rays, the second on 226 workgroups; four trips per wave in the first."""
    fwd = _circle_forward(golden_dir, 100, 10000, 8, 4, 13)
    gi, gw = _upstream(10000, 3)
    r = _check("unequal chunks 10000x8", fwd, _backward(fwd, gi, gw), gi, gw)
    assert r["geo"]["chunks"] == nb.CASES["unequal_chunks"]["chunks"]


def test_large_addends_take_the_fp32_path(golden_dir):
    """The two-chunk rays with the upstream gradients scaled by a power of two, chosen from the unscaled run's own wave sums so that the largest
    dW1 wave sum is 8 .. 16 thr_mlp: some waves' addends take sf_grad_add's fp32 atomic, most stay in fixed point, both kinds within one
    element.  (A power of two scales every fp32 value of both stages exactly.)"""
    fwd = _circle_forward(golden_dir, 64, 4096, 16, 3, 12)
    gi, gw = _upstream(4096, 2)
    geo = nb.bwd_geometry(4096, 16)
    b1 = _backward(fwd, gi, gw)
    fw1 = nb.field_forward64(fwd["feat"], fwd["W"], fwd["x"], b1["dsig"].reshape(-1), b1["drgb"].reshape(-1, 3))
    S = nb._wave_sums([(((fw1["dout"] @ fwd["W"][4].double()) * (fw1["z2"] > 0)), fw1["h1"])], geo)
    import math
    scale = 2.0 ** math.ceil(math.log2(8.0 * geo["thr"] / float(S.abs().max())))
    gi, gw = gi * scale, gw * scale
    r = _check(f"large addends 4096x16 scale 2^{int(math.log2(scale))}", fwd, _backward(fwd, gi, gw), gi, gw, geo=geo)
    n_waves = geo["n_waves"]
    sure, maybe = r["ref"]["w1"]["sure_fp32"], r["ref"]["w1"]["maybe_fp32"]
    assert int((sure > 0).sum()) > 0 and int(((sure > 0) & (maybe < n_waves)).sum()) > 0 and int((maybe == 0).sum()) > 0


def test_opaque_samples(golden_dir):
    """The golden rays' sorted depths with a synthetic sigma_s (backward only): stage A in the semi-opaque (one = a few 2^-24) and the saturated
    (one == 1e-15f, expf underflows) regime of after / (1 - alpha + 1e-15); the conditions hold on the reference alone."""
    g, p, net = _golden(golden_dir)
    fwd = _golden_forward(golden_dir)
    sigma = nb.opaque_sigma(fwd["z_s"].cpu(), fwd["nears"].cpu(), fwd["fars"].cpu(), 64, 5)
    gi, gw = g["g_image"], g["g_ws"]
    r = _check("opaque 256x64", fwd, _backward(fwd, gi, gw, sigma=sigma), gi, gw)
    semi, sat, tight = nb.opaque_conditions(r["a"])
    print(f"opaque conditions: e in [1e-6, 1e-2] {semi:.3f} one == 1e-15f {sat:.3f} bound <= 1e-4 of the ray's largest |want| {tight:.4f}")
    assert semi >= 0.05 and sat >= 0.05 and tight >= 0.9, (semi, sat, tight)


# ------------------------------------------------------------------------------------------- the table gradient of pass 0, per element
def _table_levels(name, fwd, bwd, o, d, aabb, offs, levels, gridtype, binned, e=0):
    """The table gradient of a backward on chosen levels against the float64 corner sums of ITS OWN d(feat) (read from the workspace), under
    scatter_bound: every element of the level, and the level's d(feat) not all zero.  levels: (level, merged) -- merged = k_ngp_scatter,
    which ngp_scatter_plan itself (csrc/ngp_bwd_plan.h through the harness of tests/test_hostemu_ngp_bwd.py) must give levels [0, last);
    binned: whether the plan sends the other levels to the binned scatter (else k_ngp_scatter_fine)."""
    import test_hostemu_ngp_bwd as hb
    offs = offs.to(torch.int32).cpu()
    sp = hb._c_scatter_plan(hb._lib(), offs, 16, log2_scale(), 1, fwd["N"], fwd["T"])
    assert sp["binned"] == binned and all(merged == (level < sp["last"]) for level, merged in levels), (name, sp, levels)
    for level, merged in levels:
        assert float(bwd["dfeat"][:, 2 * level:2 * level + 2].abs().max()) > 0, (name, level)
        want, sum_abs, count = sb.scatter_ref64({"encoder.offsets": offs}, o, d, aabb, fwd["z_s"].cpu(), bwd["dfeat"], level, e, gridtype=gridtype)
        nb.check_elements(f"{name} table level {level}", bwd["table"][int(offs[level]):int(offs[level + 1])], want,
                          sb.scatter_bound(want, sum_abs, count, merged))


def _large_table_net(p, gridtype):
    """the teacher's MLP behind a 2^20-row encoder with a random table (the field of tests/test_gpu_ngp.py::
    test_table_gradient_of_a_large_hash_map_keeps_the_atomic_scatter, or its `tiled` twin): outside the binned scatter"""
    from sparsefusion_amd.gridencoder import GridEncoder
    from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt
    net = NeRFNetwork(get_default_torch_ngp_opt())
    net.load_state_dict({k: p[k] for k in net.state_dict().keys()})
    net = net.to(DEV)
    enc = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=20, desired_resolution=2048 * net.bound,
                      gridtype=gridtype, align_corners=False).to(DEV)
    gen = torch.Generator().manual_seed(31)
    with torch.no_grad():
        enc.embeddings.copy_((torch.rand(enc.embeddings.shape, generator=gen) - 0.5).to(DEV))
    net.encoder, net._handle = enc, None
    offs = enc.offsets.to(torch.int32).cpu()
    assert int((offs[1:] - offs[:-1]).max()) > 1 << 19           # ngp_scatter_plan does not bin: a level beyond SB_MAX_BUCKETS buckets
    return net, offs


def _small_rays(n_side, N, T, seed):
    o, d = ngp_ref.circle_rays(n_side, view=2)
    o, d = o[:N].contiguous(), d[:N].contiguous()
    gen = torch.Generator().manual_seed(seed)
    return o, d, torch.rand(N, T, generator=gen), torch.rand(N, T, generator=gen)


@pytest.mark.parametrize("n_side,N,T,rays_per_row", [(7, 37, 11, 0), (16, 128, 20, 16)], ids=["37x11", "128x20_patches"])
def test_table_gradient_per_element_teacher(golden_dir, n_side, N, T, rays_per_row):
    """Pass 0 on the teacher field: level 0 through k_ngp_scatter (register-merged runs, the LDS cache; two 8 x 8 patches with the image
    layout) and level 8 through the binned scatter."""
    g, p, net = _golden(golden_dir)
    o, d, uc, uf = _small_rays(n_side, N, T, 40 + N)
    fwd = _forward(net, p, o, d, T, uc, uf)
    gi, gw = _upstream(N, 4)
    bwd = _backward(fwd, gi, gw, rays_per_row=rays_per_row)
    _table_levels(f"teacher {N}x{T}", fwd, bwd, o, d, p["aabb_train"], p["encoder.offsets"], ((0, True), (8, False)), gridtype=1, binned=True)


def test_table_gradient_per_element_large_hash_map(golden_dir):
    """Pass 0 on the 2^20-row `hash` field, 37 x 11: level 2 through k_ngp_scatter<1024, 0>, level 13 through k_ngp_scatter_fine<0>."""
    g, p, _ = _golden(golden_dir)
    net, offs = _large_table_net(p, 'hash')
    o, d, uc, uf = _small_rays(7, 37, 11, 51)
    fwd = _forward(net, p, o, d, 11, uc, uf)
    gi, gw = _upstream(37, 5)
    bwd = _backward(fwd, gi, gw)
    _table_levels("large hash 37x11", fwd, bwd, o, d, p["aabb_train"], offs, ((2, True), (13, False)), gridtype=0, binned=False)


def test_table_gradient_per_element_large_tiled_map(golden_dir):
    """The 2^20-row `tiled` field, 37 x 11, random sorted depths in place of the forward's (some samples leave the box; the backward
    re-gathers): levels 10 .. 15 are z-dropped and, the table being outside the bins, go through k_ngp_scatter_fine -- level 12 there and
    level 2 through k_ngp_scatter for pass 0, and level 12 of one offset pass (e = 3) for k_ngp_scatter_fine<1>."""
    from sparsefusion_amd import _lib
    g, p, _ = _golden(golden_dir)
    net, offs = _large_table_net(p, 'tiled')
    N, T, e = 37, 11, 3
    o, d, uc, uf = _small_rays(7, N, T, 52)
    fwd = _forward(net, p, o, d, T, uc, uf)
    gen = torch.Generator().manual_seed(53)
    fwd["z_s"] = (torch.rand(N, 2 * T, generator=gen) * 9.0 + 1.0).sort(1).values.contiguous().to(DEV)
    gi, gw = _upstream(N, 6)
    bwd = _backward(fwd, gi, gw, use_cache=False)
    _table_levels("large tiled 37x11", fwd, bwd, o, d, p["aabb_train"], offs, ((2, True), (12, False)), gridtype=1, binned=False)
    # one offset pass on the same field and depths
    M = N * 2 * T
    grads = [torch.zeros_like(t) for t in fwd["params"]]
    gs = _lib.SfNgpFieldGrad()
    (gs.g_embeddings, gs.g_w0, gs.g_b0, gs.g_w1, gs.g_b1, gs.g_w2, gs.g_b2) = (t.data_ptr() for t in grads)
    f = fwd["handle"].struct(fwd["params"])
    lib = _lib.lib()
    wb = lib.sf_ngp_render_workspace_bytes(N, T)
    work = torch.zeros(wb // 4, device=DEV)
    ds_e = torch.randn(N, 2 * T, generator=gen).to(DEV)
    _lib.check(lib.sf_ngp_render_offset_backward(C.byref(f), C.byref(gs), _lib.ptr(fwd["o"]), _lib.ptr(fwd["d"]), _lib.ptr(fwd["aabb"]), N, T,
                                                 _lib.ptr(fwd["z_s"]), _lib.ptr(ds_e), e, sb.EPS, 0, _lib.ptr(work), wb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    off = dict(table=grads[0].cpu(), dfeat=work[4 * M:36 * M].view(16, M, 2).permute(1, 0, 2).reshape(M, 32).cpu())
    _table_levels(f"large tiled 37x11 e={e}", fwd, off, o, d, p["aabb_train"], offs, ((12, False),), gridtype=1, binned=False, e=e)

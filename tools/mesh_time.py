"""Per-stage times of NeRFRenderer.export_mesh on the GPU (torch events around each stage, median of --reps runs after one warm-up)
next to the CPU pipeline it is tested against (scipy gaussian_filter + numpy level + tests/mesh_ref.py marching cubes) on the
same field.  One JSON line per resolution.

    python tools/mesh_time.py --res 128 256 [--reps 5] [--no-cpu] [--attrs] [--texture] [--clean]

--attrs adds, per resolution and for a fixed set of 2^20 random points, the one-launch vertex attributes (sf_ngp_point_attrs) next to
the same quantities composed from seven sf_ngp_density calls and torch glue (what the field API offered before that entry point).

--texture adds, per resolution, the one-launch texture bake of the exported mesh (sf_ngp_texture_bake, 8-bit output) at 1024^2 and
2048^2 next to the composed route: a point buffer built by torch from the atlas layout, sf_ngp_density on it, torch quantisation.

--clean adds, per resolution, the clean-up stage on the exported mesh (mesh.clean_mesh: connected components, filter count, the read
of {V', F'}, emit; and the two halves through the C ABI) next to the wall time of the scipy + numpy restatement the tests compare it
with (tests/mesh_clean_common.py), and after the resolutions one line for the synthetic 1.1 M-face case of the tests.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from ngp_common import BOUND, params_from_cfg      # noqa: E402
import mesh_ref                                    # noqa: E402
from sparsefusion_amd import mesh                  # noqa: E402
from sparsefusion_amd.nerf import NeRFNetwork, get_default_torch_ngp_opt      # noqa: E402


def gpu_run(net, R, path):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    torch.cuda.synchronize()
    ev[0].record()
    vol = mesh.density_lattice(net, R, BOUND)
    ev[1].record()
    sm, stats = mesh.smooth_gaussian(vol, 1.5, return_stats=True)
    ev[2].record()
    mean, std = (float(x) for x in stats.cpu())
    v, f = mesh.marching_cubes(sm, mean + std * 0.25)       # classify + scan, counts read back, emit
    ev[3].record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh.export_obj(v, f, path)
    t_obj = (time.perf_counter() - t0) * 1e3
    return dict(lattice=ev[0].elapsed_time(ev[1]), gauss_stats=ev[1].elapsed_time(ev[2]), mc=ev[2].elapsed_time(ev[3]), obj=t_obj,
                V=int(v.shape[0]), F=int(f.shape[0])), vol


def mc_split(sm, iso):
    """classify + scan and emit timed separately through the C ABI (the same calls marching_cubes makes)."""
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    nx, ny, nz = sm.shape
    wb = lib.sf_mc_workspace_bytes(nx, ny, nz)
    work = torch.empty(wb, dtype=torch.uint8, device=sm.device)
    counts = torch.empty(2, dtype=torch.int32, device=sm.device)
    st = _lib.stream_ptr()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    _lib.check(lib.sf_mc_count(_lib.ptr(sm), nx, ny, nz, iso, _lib.ptr(work), wb, _lib.ptr(counts), st))
    e[1].record()
    V, F = (int(c) for c in counts.cpu())
    verts = torch.empty(V, 3, device=sm.device)
    faces = torch.empty(F, 3, dtype=torch.int32, device=sm.device)
    e2 = torch.cuda.Event(enable_timing=True)
    e2.record()
    _lib.check(lib.sf_mc_emit(_lib.ptr(sm), nx, ny, nz, iso, _lib.ptr(work), wb, _lib.ptr(verts), _lib.ptr(faces), st))
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e2.elapsed_time(e[2])


def _median_ms(fn, reps):
    times = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def attrs_time(net, x, eps, reps):
    """ms of one sf_ngp_point_attrs launch (albedo + normal) and of the composition from seven sf_ngp_density calls on x [P, 3]"""
    from sparsefusion_amd.nerf.utils import safe_normalize

    def composed():
        albedo = net.density(x)["albedo"]
        comps = []
        for a in range(3):
            o = torch.zeros(1, 3, device=x.device)
            o[0, a] = eps
            sp = net.density((x + o).clamp(-BOUND, BOUND))["sigma"]
            sn = net.density((x - o).clamp(-BOUND, BOUND))["sigma"]
            comps.append(0.5 * (sp - sn) / eps)
        n = safe_normalize(torch.stack(comps, -1))
        n[torch.isnan(n)] = 0
        return albedo, n

    return dict(P=int(x.shape[0]), eps=float(eps), one_launch_ms=_median_ms(lambda: mesh.vertex_attributes(net, x, eps), reps),
                seven_density_calls_ms=_median_ms(composed, reps))


def texture_time(net, verts, faces, W, reps):
    """ms of one sf_ngp_texture_bake launch (rgb8 only) and of the composed route on the same mesh.  The texel -> (face, barycentric
    numerators) table of the composed route depends on (F, W) alone and is built once, outside the timing."""
    import texture_common as tc
    F = int(faces.shape[0])
    G, c = mesh.atlas_layout(F, W)
    dev = verts.device
    face_id, _ = tc.np_bake_points(np.zeros((1, 3), np.float32), np.zeros((F, 3), np.int64), W)
    used = torch.from_numpy(face_id.reshape(-1) >= 0).to(dev)
    fid = torch.from_numpy(face_id.reshape(-1).astype(np.int64)).to(dev)[used]
    t = torch.nonzero(used).squeeze(1)
    x, y = t % W, t // W
    i, j = x % c, y % c
    upper = (fid & 1) == 1
    i, j = torch.where(upper, c - 1 - i, i), torch.where(upper, c - 1 - j, j)
    leg = c - 5
    p, q = (i - 1).clamp(0, leg), (j - 1).clamp(0, leg)
    e = (p + q - leg).clamp(min=0)
    u, v = ((p - (e + 1) // 2).float() / leg)[:, None], ((q - e // 2).float() / leg)[:, None]

    def composed():
        tri = verts[faces.long()[fid]]                                # [n, 3, 3]
        pts = ((1.0 - u) - v) * tri[:, 0] + u * tri[:, 1] + v * tri[:, 2]
        a = net.density(pts)["albedo"]
        img = torch.zeros(W * W, 3, dtype=torch.uint8, device=dev)
        img[used] = (a.clamp(0, 1) * 255).to(torch.uint8)
        return img.view(W, W, 3)

    return dict(W=W, F=F, cell=c, texels_used=int(used.sum()), one_launch_ms=_median_ms(lambda: mesh.bake_texture(net, verts, faces, W), reps),
                composed_ms=_median_ms(composed, reps))


def clean_time(verts, faces, reps, min_faces=8, min_fraction=0.0):
    """ms of mesh.clean_mesh (with its read-back), of sf_mesh_components and of sf_mesh_filter_count + emit on their own (events
    around the C entries, outputs sized for the full mesh so that no read-back sits inside), and the wall ms of the CPU restatement"""
    import mesh_clean_common as mcc
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    V, F, dev = int(verts.shape[0]), int(faces.shape[0]), verts.device
    i32 = dict(dtype=torch.int32, device=dev)
    vl, fl, per, c3, c2 = (torch.empty(n, **i32) for n in (V, F, V, 3, 2))
    wc, wf = lib.sf_mesh_components_workspace_bytes(V, F), lib.sf_mesh_filter_workspace_bytes(V, F)
    ws_c, ws_f = (torch.empty(n, dtype=torch.uint8, device=dev) for n in (wc, wf))
    ov, of, vi, fi = torch.empty(V, 3, device=dev), torch.empty(F, 3, **i32), torch.empty(V, **i32), torch.empty(F, **i32)
    P, st = _lib.ptr, _lib.stream_ptr()

    def components():
        _lib.check(lib.sf_mesh_components(P(faces), F, V, P(vl), P(fl), P(per), P(c3), P(ws_c), wc, st))

    def filt():
        _lib.check(lib.sf_mesh_filter_count(P(faces), F, V, P(vl), P(per), P(c3), min_faces, min_fraction, P(ws_f), wf, P(c2), st))
        _lib.check(lib.sf_mesh_filter_emit(P(verts), P(faces), F, V, P(ws_f), wf, P(ov), P(of), P(vi), P(fi), st))

    out = dict(V=V, F=F, min_faces=min_faces, min_fraction=min_fraction,
               clean_mesh_ms=_median_ms(lambda: mesh.clean_mesh(verts, faces, min_faces, min_fraction), reps),
               components_ms=_median_ms(components, reps), filter_count_emit_ms=_median_ms(filt, reps))
    n_comp, largest, n_invalid = (int(x) for x in c3.cpu())
    V2, F2 = (int(x) for x in c2.cpu())
    out.update(n_components=n_comp, largest=largest, n_invalid=n_invalid, V_kept=V2, F_kept=F2)
    vh, fh = verts.cpu().numpy(), faces.cpu().numpy()
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = mcc.reference_components(fh, V)
        t1 = time.perf_counter()
        mcc.reference_clean(vh, fh, V, ref, min_faces, min_fraction)
        cpu.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    out["cpu_scipy_components_ms"], out["cpu_numpy_filter_ms"] = (statistics.median(c[k] for c in cpu) for k in (0, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--attrs", action="store_true")
    ap.add_argument("--texture", action="store_true")
    ap.add_argument("--clean", action="store_true")
    a = ap.parse_args()
    golden = torch.load(os.path.join(ROOT, "tests", "golden", "ngp_render.pt"))
    p = params_from_cfg(golden["teacher"]["cfg"])
    net = NeRFNetwork(get_default_torch_ngp_opt())
    net.load_state_dict({k: p[k] for k in net.state_dict().keys()})
    net = net.to("cuda:0").eval()
    tmp = tempfile.mkdtemp()
    for R in a.res:
        runs = []
        with torch.no_grad():
            for i in range(a.reps + 1):
                r, vol = gpu_run(net, R, os.path.join(tmp, "m.obj"))
                if i:
                    runs.append(r)
            sm, stats = mesh.smooth_gaussian(vol, 1.5, return_stats=True)
            iso = float(stats[0] + 0.25 * stats[1])
            splits = [mc_split(sm, iso) for _ in range(a.reps + 1)][1:]
            t0 = time.perf_counter()
            net.export_mesh(tmp, resolution=R)
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
        med = {k: statistics.median(r[k] for r in runs) for k in ("lattice", "gauss_stats", "mc", "obj")}
        out = dict(R=R, gpu_ms=dict(lattice=med["lattice"], gauss_stats=med["gauss_stats"],
                                    classify_scan=statistics.median(s[0] for s in splits), emit=statistics.median(s[1] for s in splits),
                                    mc_with_readback=med["mc"]), obj_write_ms=med["obj"], export_mesh_wall_ms=total,
                   V=runs[0]["V"], F=runs[0]["F"])
        if a.attrs:
            with torch.no_grad():
                verts, _ = net.export_mesh(tmp, resolution=R)
                eps = 2.0 * BOUND / (R - 1)
                g = torch.Generator().manual_seed(3)
                rand = ((torch.rand(1 << 20, 3, generator=g) * 2 - 1) * BOUND).to(verts.device)
                out["attrs_vertices"] = attrs_time(net, verts.contiguous(), eps, a.reps)
                out["attrs_random"] = attrs_time(net, rand, eps, a.reps)
        if a.texture:
            with torch.no_grad():
                verts, faces = net.export_mesh(tmp, resolution=R)
                out["texture"] = [texture_time(net, verts.contiguous(), faces, W, a.reps) for W in (1024, 2048)]
        if a.clean:
            with torch.no_grad():
                verts, faces = net.export_mesh(tmp, resolution=R)
                out["clean"] = clean_time(verts.contiguous(), faces, a.reps)
        if not a.no_cpu:
            v = vol.cpu().numpy()
            t0 = time.perf_counter()
            s64 = mesh_ref.smooth_gaussian(v, 1.5)
            t1 = time.perf_counter()
            lvl = mesh_ref.iso_level(s64)
            t2 = time.perf_counter()
            cv, cf = mesh_ref.marching_cubes(s64.astype(np.float32), lvl)
            t3 = time.perf_counter()
            out["cpu_ms"] = dict(gaussian=(t1 - t0) * 1e3, stats=(t2 - t1) * 1e3, marching_cubes=(t3 - t2) * 1e3)
            out["cpu_V"], out["cpu_F"] = int(cv.shape[0]), int(cf.shape[0])
        print(json.dumps(out), flush=True)
    if a.clean:
        import mesh_clean_common as mcc
        c = mcc.make_case(mcc.BIG_CASE)
        verts, faces = torch.tensor(c["vertices"]).to("cuda:0"), torch.tensor(c["faces"]).to("cuda:0")
        print(json.dumps(dict(case="synthetic strips, permuted numbering", clean=clean_time(verts, faces, a.reps))), flush=True)


if __name__ == "__main__":
    main()

"""Per-element parity of the normalisation / softmax / pack kernels of csrc/unet_ops.hip on the shapes the SD-VAE and the B >= 8 UNet
plans run them at (GroupNorm with 32 groups of 4 .. 16 channels, eps 1e-6, with and without SiLU; the per-sample attention of the VAE's
AttnBlock) -- every branch of run_gn, each of the six k_gn_one instantiations, ELTWISE modes 5 and 6 and OP_GN_FINALIZE through the
C-ABI plan executor, against the float64 references and the derived bounds of tests/norm_cases.py.  Every case prints its margin line
(profiles/norm_parity_margins.log)."""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc
from norm_cases import U24, mkop, run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OLD = (1.2e-2, 1e-2)          # the whole-tensor allclose of test_gpu_unet_ops.py::test_gn_act, printed beside the new figures


def bf(t):
    return t.to(torch.bfloat16).float()


def ulp32(s):
    """One fp32 ulp at the magnitude s (float64 tensor)."""
    return torch.exp2((torch.frexp(s)[1].double() - 1).clamp(min=-126.0) - 23)


def _source(kind, B, HW, C, Cg, g):
    rn = lambda *s: torch.randn(*s, generator=g)
    if kind == "tiny_var":                  # group variance ~ 1e-6 = eps: an eps of 1e-5 would move every output by a factor of about 2
        return rn(B, HW, C) * 1e-3
    if kind == "mean8":                     # mean of 8 sigma: E[x^2] / var = 65, the cancellation case of the one-pass variance
        return rn(B, HW, C) + 8.0
    x = rn(B, HW, C) * 2 + 0.5
    if kind == "const_group":               # group 1 of image 0 is constant (0.5: every fp32 partial sum is exact): var = 0 exactly, the clamp, beta out
        x[0, :, Cg:2 * Cg] = 0.5
    return x


def _lazy_source(mode, B, HW, C1, g, variant):
    """(float64 value, uncertainty, summed magnitudes, op operands p[8..10], (mode, groups, npad), initial p[0])."""
    rn = lambda *s: torch.randn(*s, generator=g)
    M = B * HW
    if mode == 1:
        # split-K partials: bias + sum of slabs + residual.  The write-back is held to ONE fp32 ulp of the summed magnitudes, which covers two
        # roundings (each at most half an ulp of a partial sum that is no larger than the summed magnitudes): so a case has at most three
        # terms -- "both": bias + 1 slab + residual, "bias": bias + 2 slabs, "resid": 2 slabs + residual, "bare": 2 slabs (0 + slab is exact)
        groups, npad = (1, C1 + 16) if variant == "both" else (2, C1 + 16 if variant == "resid" else C1 + 4)
        ws = rn(groups, M, npad)
        bias = rn(C1) if variant in ("both", "bias") else None
        r = rn(M, C1) if variant in ("both", "resid") else None
        x64 = ws[:, :, :C1].double().sum(0)
        mag = ws[:, :, :C1].double().abs().sum(0)
        if bias is not None:
            x64, mag = x64 + bias.double(), mag + bias.double().abs()
        if r is not None:
            x64, mag = x64 + r.double(), mag + r.double().abs()
        return x64, (groups + 1) * U24 * mag, mag, (ws, bias, r), (1, groups, npad), torch.full((M, C1), float("nan"))
    h, gate, r = rn(M, C1), torch.sigmoid(rn(B, C1)), rn(M, C1)          # gate: h * gate + r; variant: r given, else the destination holds it
    hg = h.double() * gate.double().repeat_interleave(HW, 0)
    x64, mag = hg + r.double(), hg.abs() + r.double().abs()
    return x64, 2 * U24 * mag, mag, (h, gate, r if variant else None), (2, 0, 0), (torch.full((M, C1), float("nan")) if variant else r.clone())


def run_gn_case(name, B, HW, C1, C2=0, G=32, flags=(0, 4, 8), expect=None, silu=True, eps=1e-6, ss=False, raw=True, kind="normal",
                lazy=0, variant="both", seed=0):
    """One OP_GN_ACT shape under each dispatch flag (0: run_gn's rule, 4: k_gn_stats(_px) + k_gn_apply, 8: k_gn_one): every run must meet the
    per-element bound.  expect: kernel name per flag (the branch of run_gn the case is written for)."""
    g = torch.Generator().manual_seed(seed + B + HW + C1 + 3 * C2)
    rn = lambda *s: torch.randn(*s, generator=g)
    C, M = C1 + C2, B * HW
    Cg = C // G
    s2_scale = 2 ** -0.5
    if lazy:
        x64, dx1, mag, lz_p, lz_i, p0_init = _lazy_source(lazy, B, HW, C1, g, variant)
        x64, dx1 = x64.view(B, HW, C1), dx1.view(B, HW, C1)
    else:
        x1 = _source(kind, B, HW, C1, Cg, g)
        x64, dx1, lz_p, lz_i = x1.double(), None, (None, None, None), (0, 0, 0)
    x2 = rn(B, HW, C2) if C2 else None
    gamma, beta = 1 + 0.2 * rn(C), 0.2 * rn(C)
    ss_stride = 3 * C + 8                                    # != 2 C: the block's slice starts at column C of a wider row
    ss_all = rn(B, ss_stride) * 0.3
    ssv = (ss_all[:, C:2 * C], ss_all[:, 2 * C:3 * C]) if ss else None
    d = lambda t: None if t is None else t.to(DEV)
    x2d, gd, bd, ssd, lzd = d(x2), d(gamma), d(beta), d(ss_all), tuple(d(t) for t in lz_p)
    x1d = None if lazy else d(x1)
    xc_raw = torch.cat([x64.float(), x2 * torch.tensor(nc.f32(s2_scale))], -1) if C2 else x64.float()
    refs = {}
    for fl in flags:
        geo = nc.gn_geometry(B, HW, C1, C2, G, fl, lazy)
        if expect is not None:
            assert geo["kernel"] == expect[fl] or (isinstance(expect[fl], tuple) and (geo["kernel"], geo["NT"], geo["NCH"]) == expect[fl]), (name, fl, geo)
        counts = nc.stat_counts(geo)
        if counts not in refs:
            refs[counts] = nc.gn_act_ref64(x64, x2, s2_scale, G, gamma, beta, eps, counts, ss=ssv, silu=silu, dx1=dx1)
        want, delta, sums, sums_bound = refs[counts]
        if lazy:
            x1d = d(p0_init.clone())
        out = torch.full((B, HW, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        rawd = torch.full((B, HW, C), float("nan"), dtype=torch.bfloat16, device=DEV) if raw else None
        one = geo["kernel"] == "k_gn_one"
        stats = torch.full((B * G * 2,), 7.0 if one else 0.0, dtype=torch.float64, device=DEV)      # the pair adds into a zeroed buffer
        rc = run([mkop(nc.OP_GN_ACT, fl | (0 if silu else 1),
                       p=(x1d, x2d, gd, bd, (ssd.data_ptr() + C * 4) if ss else None, out, rawd, stats) + lzd,
                       i=(B, HW, C1, C2, ss_stride) + lz_i + (G,), f=(eps, s2_scale))])
        assert rc == 0, f"{name}: op refused ({rc})"
        tag = f"gn_act {name} flags {fl} {geo['kernel']}" + (f"<{geo['NT']},{geo['NCH']}>" if one else "")
        nc.check_bf16(tag, out.cpu(), want, delta, old=OLD if silu else None)
        if kind == "const_group":      # variance exactly 0 -> the clamp -> (v - mean) = 0: the group's output is beta (through scale / shift / SiLU), rounded, whatever rstd is
            blk = want[0, :, Cg:2 * Cg]
            assert not ss and not silu and torch.equal(blk, beta[Cg:2 * Cg].double().expand(HW, Cg)), "the reference of the constant group is not beta"
            assert torch.equal(out.cpu()[0, :, Cg:2 * Cg], blk.float().to(torch.bfloat16)), f"{tag}: a constant group must give beta"
        if raw and not lazy:
            assert torch.equal(rawd.cpu(), xc_raw.to(torch.bfloat16)), f"{tag}: raw copy != bf16(source)"
        if one:        # k_gn_one keeps its statistics in the workgroup and leaves p[7] as it found it (no consumer reads it: unet_ops.hip GN_ACT comment)
            assert bool((stats == 7.0).all()), f"{tag}: k_gn_one wrote the statistics buffer"
        else:
            nc.check_stats(tag, stats.cpu(), sums, sums_bound)
        if lazy:       # the materialised first source: the float64 value of the same expression to 1 fp32 ulp of the summed magnitudes
            got0 = x1d.cpu().double()
            assert bool(((got0 - x64.view(M, C1)).abs() <= ulp32(mag)).all()), \
                f"{tag}: materialised source off by {float(((got0 - x64.view(M, C1)).abs() / ulp32(mag)).max()):.3g} ulp of the summed magnitudes"
            if raw:
                rr = rawd.cpu()[..., :C1].reshape(M, C1)
                assert torch.equal(rr, x1d.cpu().to(torch.bfloat16)), f"{tag}: raw copy != bf16(materialised source)"
    return refs


ONE, PX, ST = "k_gn_one", "k_gn_stats_px", "k_gn_stats"

# name -> kwargs.  B, HW, C, G = 32 unless said; chunks = HW * (C / G) / 4 picks the k_gn_one instantiation.
GN_ONE_CASES = {
    # the six k_gn_one instantiations at G = 32, B = 8 (B * G = 256 workgroups: taken by the rule); flag 4: the pair (k_gn_stats_px: Cg <= 16)
    "one_256x2_b8_hw256_c256": dict(B=8, HW=256, C1=256, expect={0: (ONE, 256, 2), 4: PX, 8: (ONE, 256, 2)}, ss=True),
    "one_256x4_b8_hw256_c512": dict(B=8, HW=256, C1=512, expect={0: (ONE, 256, 4), 4: PX, 8: (ONE, 256, 4)}),
    "one_256x8_b8_hw1024_c256": dict(B=8, HW=1024, C1=256, expect={0: (ONE, 256, 8), 4: PX, 8: (ONE, 256, 8)}, silu=False),
    "one_256x16_b8_hw1024_c512_vae_32x32": dict(B=8, HW=1024, C1=512, expect={0: (ONE, 256, 16), 4: PX, 8: (ONE, 256, 16)}),
    "one_1024x8_b8_hw4096_c256": dict(B=8, HW=4096, C1=256, expect={0: (ONE, 1024, 8), 4: PX, 8: (ONE, 1024, 8)}),
    "one_1024x16_b8_hw4096_c512": dict(B=8, HW=4096, C1=512, expect={0: (ONE, 1024, 16), 4: PX, 8: (ONE, 1024, 16)}, raw=False),
    # 36 chunks: one partial wave of <256, 2> does the work, the other threads are idle
    "one_idle_threads_b8_hw36_c128": dict(B=8, HW=36, C1=128, expect={0: (ONE, 256, 2), 4: PX, 8: (ONE, 256, 2)}, ss=True),
    # the boundary: exactly 1024 * 16 chunks still fit; twice that must fall back to the pair even under flag 8
    "one_boundary_16384_chunks_b8_hw16384_c128": dict(B=8, HW=16384, C1=128, expect={0: (ONE, 1024, 16), 4: PX, 8: (ONE, 1024, 16)}, raw=False),
    "one_over_boundary_falls_back_b8_hw16384_c256": dict(B=8, HW=16384, C1=256, flags=(0, 8), expect={0: PX, 8: PX}, raw=False),
    # the second rule (flags 0): B * G >= 64 and at most 2^19 elements -- one case on each side (Cg = 32: the pair is k_gn_stats)
    "one_second_rule_inside_b2_hw256_c1024": dict(B=2, HW=256, C1=1024, expect={0: (ONE, 256, 8), 4: ST, 8: (ONE, 256, 8)}),
    "one_second_rule_outside_b2_hw320_c1024": dict(B=2, HW=320, C1=1024, expect={0: ST, 4: ST, 8: (ONE, 256, 16)}),
    # G = 8 (op field i[8] = 8), two sources: the UNet's form on the same bound
    "one_g8_concat_b32_hw64_c1024_512": dict(B=32, HW=64, C1=1024, C2=512, G=8, eps=1e-5, expect={0: (ONE, 256, 16), 4: ST, 8: (ONE, 256, 16)}, ss=True),
}

GN_PX_CASES = {
    # k_gn_stats_px: single plain source, Cg <= 16, C / 4 divides 256; slabs = HW / (ppi * 16) from 1 to the 1024 cap
    "px_one_slab_b1_hw64_c128": dict(B=1, HW=64, C1=128, flags=(0, 8), expect={0: PX, 8: (ONE, 256, 2)}),
    "px_c256_b1_hw1024": dict(B=1, HW=1024, C1=256, flags=(0, 8), expect={0: PX, 8: (ONE, 256, 8)}, ss=True),
    "px_c512_b2_hw4096": dict(B=2, HW=4096, C1=512, flags=(0, 8), expect={0: PX, 8: (ONE, 1024, 16)}, silu=False),
    "px_c1024_cg32_is_not_px_b1_hw256": dict(B=1, HW=256, C1=1024, flags=(0, 8), expect={0: ST, 8: (ONE, 256, 8)}),      # Cg = 32 > 16: k_gn_stats
    "px_c1024_g64_b1_hw1024": dict(B=1, HW=1024, C1=1024, G=64, flags=(0, 8), expect={0: PX, 8: (ONE, 256, 16)}),       # ppi = 1: one pixel per pass
    "px_512_slabs_b1_hw65536_c128": dict(B=1, HW=65536, C1=128, flags=(0,), expect={0: PX}, raw=False),
    "px_slab_cap_b1_hw65536_c512": dict(B=1, HW=65536, C1=512, flags=(0,), expect={0: PX}, raw=False),
    # HW not a multiple of ppi * 16 (ppi = 8 at C = 128: 1000 = 7 slabs of 143 pixels, the last one short and ragged against ppi)
    "px_ragged_b1_hw1000_c128": dict(B=1, HW=1000, C1=128, flags=(0, 8), expect={0: PX, 8: (ONE, 256, 4)}, ss=True),
}

GN_STATS_CASES = {
    # k_gn_stats with G = 32: C = 384 (c4 = 96 does not divide 256), a two-source concat with src2_scale, the small-map slice rule
    "stats_c384_b2_hw1024": dict(B=2, HW=1024, C1=384, flags=(0, 8), expect={0: ST, 8: (ONE, 256, 16)}),
    "stats_concat_b2_hw1024_c256_256": dict(B=2, HW=1024, C1=256, C2=256, flags=(0, 8), expect={0: ST, 8: (ONE, 256, 16)}, ss=True),
    "stats_small_map_slices_b1_hw256_c512": dict(B=1, HW=256, C1=384, C2=128, flags=(0, 8), expect={0: ST, 8: (ONE, 256, 4)}),      # 1024 chunks: want = 128 / 32 = 4 slices where the 2048-chunk rule gives 1
    "stats_long_slices_b1_hw16384_c384": dict(B=1, HW=16384, C1=384, flags=(0,), expect={0: ST}, raw=False),                       # 24 slices of 2048 chunks
}

GN_LAZY_CASES = {
    # lazy first source, materialised by the statistics pass: mode 1 (split-K partials; bias and residual present or not, npad > C), mode 2
    # (gate; residual given, and the destination as residual), on the pair (k_gn_stats: a lazy source never takes k_gn_stats_px) and on k_gn_one
    "lazy_splitk_bias_resid_b8_hw64_c256": dict(B=8, HW=64, C1=256, lazy=1, variant="both", expect={0: (ONE, 256, 2), 4: ST, 8: (ONE, 256, 2)}),
    "lazy_splitk_bare_b2_hw256_c512": dict(B=2, HW=256, C1=512, lazy=1, variant="bare", flags=(4, 8), expect={4: ST, 8: (ONE, 256, 4)}, ss=True),
    "lazy_splitk_concat_g8_b8_hw16_c1024_1024": dict(B=8, HW=16, C1=1024, C2=1024, G=8, eps=1e-5, lazy=1, variant="resid", expect={0: (ONE, 256, 4), 4: ST, 8: (ONE, 256, 4)}),
    "lazy_splitk_bias_b8_hw256_c256": dict(B=8, HW=256, C1=256, lazy=1, variant="bias", expect={0: (ONE, 256, 2), 4: ST, 8: (ONE, 256, 2)}, ss=True),
    "lazy_gate_resid_b8_hw64_c256": dict(B=8, HW=64, C1=256, lazy=2, variant=True, expect={0: (ONE, 256, 2), 4: ST, 8: (ONE, 256, 2)}, silu=False),
    "lazy_gate_dst_resid_b2_hw256_c512": dict(B=2, HW=256, C1=512, lazy=2, variant=False, flags=(4, 8), expect={4: ST, 8: (ONE, 256, 4)}),
}

GN_EDGE_CASES = {
    # no SiLU (flag 1: the VAE's AttnBlock), eps 1e-6 at a group variance of ~1e-6, a constant group, a mean of 8 sigma; raw and ss on and off
    "edge_no_silu_b2_hw1024_c512": dict(B=2, HW=1024, C1=512, silu=False, expect={0: PX, 4: PX, 8: (ONE, 256, 16)}, raw=False),
    "edge_variance_near_eps_b2_hw1024_c512": dict(B=2, HW=1024, C1=512, kind="tiny_var", expect={0: PX, 4: PX, 8: (ONE, 256, 16)}),
    "edge_variance_near_eps_no_silu_b8_hw256_c256": dict(B=8, HW=256, C1=256, kind="tiny_var", silu=False, expect={0: (ONE, 256, 2), 4: PX, 8: (ONE, 256, 2)}, ss=True),
    "edge_constant_group_b2_hw1024_c256": dict(B=2, HW=1024, C1=256, kind="const_group", silu=False, expect={0: (ONE, 256, 8), 4: PX, 8: (ONE, 256, 8)}),      # (2^19 elements on 64 workgroups: the second rule)
    "edge_constant_group_g8_b2_hw256_c512": dict(B=2, HW=256, C1=512, G=8, kind="const_group", silu=False, expect={0: ST, 4: ST, 8: (ONE, 256, 16)}),
    "edge_mean_8_sigma_b2_hw1024_c512": dict(B=2, HW=1024, C1=512, kind="mean8", expect={0: PX, 4: PX, 8: (ONE, 256, 16)}, ss=True),
    "edge_mean_8_sigma_g8_b8_hw64_c1024": dict(B=8, HW=64, C1=1024, G=8, eps=1e-5, kind="mean8", expect={0: (ONE, 256, 8), 4: ST, 8: (ONE, 256, 8)}),
}


@pytest.mark.parametrize("name", list(GN_ONE_CASES))
def test_gn_act_one_launch(name):
    run_gn_case(name, **GN_ONE_CASES[name])


@pytest.mark.parametrize("name", list(GN_PX_CASES))
def test_gn_act_stats_px(name):
    run_gn_case(name, **GN_PX_CASES[name])


@pytest.mark.parametrize("name", list(GN_STATS_CASES))
def test_gn_act_stats(name):
    run_gn_case(name, **GN_STATS_CASES[name])


@pytest.mark.parametrize("name", list(GN_LAZY_CASES))
def test_gn_act_lazy_source(name):
    run_gn_case(name, **GN_LAZY_CASES[name])


@pytest.mark.parametrize("name", list(GN_EDGE_CASES))
def test_gn_act_edges(name):
    run_gn_case(name, **GN_EDGE_CASES[name])


@pytest.mark.parametrize("sel", [1, 3, 6])
@pytest.mark.parametrize("cg", [4, 8, 16])
def test_gn_act_ready_statistics_chain(cg, sel):
    """The three ops _VaePlan.resnet_block emits: a 3x3 conv whose epilogue leaves per-(tile, group) partial sums (flag 128; tile selectors
    1 / 3 / 6 = k_conv_lds / k_conv_glds / k_conv3_halo), OP_GN_FINALIZE, OP_GN_ACT with flag 2 (no statistics pass) -- against the float64
    GroupNorm of the conv output AS READ BACK; the finalised sums against the float64 sums of that output."""
    G, B, H = 32, 2, 16
    C, Cin, HW = G * cg, 64, H * H
    g = torch.Generator().manual_seed(100 * cg + sel)
    rn = lambda *s: torch.randn(*s, generator=g)
    w, bias, x = rn(C, Cin, 3, 3) / (Cin * 9) ** 0.5, rn(C), rn(B, Cin, H, H) + 0.3
    wp, cpad = nc.pack_conv(w, DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
    gamma, beta = 1 + 0.2 * rn(C), 0.2 * rn(C)
    M = B * HW
    for silu in (True, False):
        h = torch.full((B, HW, C), float("nan"), device=DEV)
        part = torch.full((M // 128, G, 2), float("nan"), dtype=torch.float64, device=DEV)
        stats = torch.zeros(B * G * 2, dtype=torch.float64, device=DEV)
        out = torch.full((B, HW, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        conv = mkop(nc.OP_CONV, 128, p=(xd, wp, bias.to(DEV), h, None, None, part),
                    i=(B, H, H, cpad, H, H, C, C, 0, 3, 3, 1, 1, 1, 256 + 16 * sel + 8, cg))
        fin = mkop(nc.OP_GN_FINALIZE, 0, p=(part, stats), i=(B, HW // 128, G))
        act = mkop(nc.OP_GN_ACT, 2 | (0 if silu else 1), p=(h, None, gamma.to(DEV), beta.to(DEV), None, out, None, stats),
                   i=(B, HW, C, 0, 0, 0, 0, 0, G), f=(1e-6, 1.0))
        assert run([conv, fin, act]) == 0
        hb = h.cpu()
        assert bool(torch.isfinite(hb).all()) and float(hb.abs().max()) > 0
        want, delta, sums, sums_bound = nc.gn_act_ref64(hb.double(), None, 1.0, G, gamma, beta, 1e-6, nc.READY_COUNTS, silu=silu)
        tag = f"gn_act ready cg {cg} conv selector {sel} silu {int(silu)}"
        nc.check_stats(tag, stats.cpu(), sums, sums_bound)
        nc.check_bf16(tag, out.cpu(), want, delta, old=OLD if silu else None)


def test_gn_act_ready_statistics_refuse_second_or_lazy_source():
    """Flag 2 (ready-made statistics) with a second source, or with a lazy first one, is refused with the op's error, not run."""
    from sparsefusion_amd import _lib
    B, HW, C, G = 1, 128, 128, 32
    x = torch.randn(B, HW, C, device=DEV)
    ga, be = torch.ones(2 * C, device=DEV), torch.zeros(2 * C, device=DEV)
    out = torch.zeros(B, HW, 2 * C, dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros(B * G * 2, dtype=torch.float64, device=DEV)
    rc = run([mkop(nc.OP_GN_ACT, 2, p=(x, x, ga, be, None, out, None, stats), i=(B, HW, C, C, 0, 0, 0, 0, G), f=(1e-6, 1.0))])
    assert rc != 0 and "ready-made statistics" in _lib.lib().sf_last_error().decode()
    rc = run([mkop(nc.OP_GN_ACT, 2, p=(x, None, ga, be, None, out, None, stats, x, x[0, 0], None), i=(B, HW, C, 0, 0, 2, 0, 0, G), f=(1e-6, 1.0))])
    assert rc != 0 and "ready-made statistics" in _lib.lib().sf_last_error().decode()
    assert float(out.float().abs().max()) == 0          # nothing ran


# ---------------------------------------------------------------------------------------------------------------------------------
# The VAE attention ops: ELTWISE mode 5 (k_pack_act), mode 6 (k_softmax_rows), and the two w_ptr convs that consume them
def _unpack_index(N, K):
    """(n, c) of every element of the packed B operand: [n_frag][k chunk][lane][8], element (lane, j) = W[nf*16 + (lane & 15)][ks*32 + 8*(lane >> 4) + j]."""
    nfr, kch = (N + 15) // 16, (K + 31) // 32
    nf, ks, lane, j = torch.meshgrid(torch.arange(nfr), torch.arange(kch), torch.arange(64), torch.arange(8), indexing="ij")
    return (nf * 16 + (lane & 15)).reshape(-1), (ks * 32 + 8 * (lane >> 4) + j).reshape(-1)


@pytest.mark.parametrize("T", [0, 1])
@pytest.mark.parametrize("K", [32, 72, 512, 1024])
@pytest.mark.parametrize("N", [16, 40, 1024])
def test_pack_act_is_bytewise_conv_pack_weights(N, K, T):
    """k_pack_act (an fp32 activation matrix -> the B operand of the conv kernels) byte for byte against the host packer
    sf_conv_pack_weights on the same matrix, plain (T = 0: src[n * ld + c]) and transposed (T = 1: src[c * ld + n]), row stride ld larger
    than the row; N padded to 16 and K to 32 with zeros; and against the layout rule itself, element by element."""
    from sparsefusion_amd import _lib
    g = torch.Generator().manual_seed(N + 3 * K + T)
    rows, cols = (K, N) if T else (N, K)
    ld = cols + 12
    src = torch.randn(rows, ld, generator=g)
    w = (src[:, :cols].t() if T else src[:, :cols]).contiguous()              # W[n][c]
    want, cpad = nc.pack_conv(w.reshape(N, K, 1, 1), "cpu")
    n_el = _lib.lib().sf_conv_packed_elems(N, cpad, 1, 1)
    assert n_el == (N + 15) // 16 * ((K + 31) // 32) * 64 * 8 == want.numel()
    out = torch.full((n_el,), 0x7fc0, dtype=torch.int16, device=DEV)          # NaN pattern: an element the kernel skips shows
    assert run([mkop(nc.OP_ELTWISE, 5, p=(src.to(DEV), None, None, out), i=(N, K, ld, T))]) == 0
    got = out.cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {n_el} packed elements differ from sf_conv_pack_weights"
    n, c = _unpack_index(N, K)
    live = (n < N) & (c < K)
    vals = got.view(torch.bfloat16)
    assert bool((got[~live] == 0).all()), "pad lanes not zero"
    assert torch.equal(vals[live], w[n[live], c[live]].to(torch.bfloat16))


def _softmax_rows_input(N, g):
    """24 rows: plain, scale * x up to +/- 80 (the max subtraction), an all-equal row, a row whose maximum is its last element."""
    x = torch.randn(24, N, generator=g) * 8
    x[4:8] *= 10
    x[4:8] = x[4:8].clamp(-640, 640)          # scale = 1/8: +/- 80
    x[4, 0], x[4, 1] = 640.0, -640.0
    x[8] = 3.25
    x[9, -1] = x[9].max() + 16.0
    x[10] = -x[9]
    return x


@pytest.mark.parametrize("N", [32, 200, 256, 1000, 1024])
def test_softmax_rows(N):
    """k_softmax_rows (ELTWISE mode 6) for any N, per element against the float64 softmax with the bf16 bound; every row's bf16 sum within
    N * 2^-9 of 1 (a half ulp of a value below 1 per element)."""
    g = torch.Generator().manual_seed(N)
    x, scale = _softmax_rows_input(N, g), 0.125
    out = torch.full(x.shape, float("nan"), dtype=torch.bfloat16, device=DEV)
    assert run([mkop(nc.OP_ELTWISE, 6, p=(x.to(DEV), None, None, out), i=(x.shape[0], N), f=(scale,))]) == 0
    want, delta = nc.softmax_ref64(x, scale)
    got = out.cpu()
    nc.check_bf16(f"softmax_rows N {N}", got, want, delta)
    assert bool(((got.double().sum(1) - 1).abs() <= N * 2.0 ** -9).all()), float((got.double().sum(1) - 1).abs().max())
    if N & (N - 1) == 0:                     # the all-equal row: exactly 1 / N where that is a power of two
        assert torch.equal(got[8], torch.full((N,), 1.0 / N).to(torch.bfloat16))


@pytest.mark.parametrize("HW,C,tile", [(1024, 512, 256 + 16 * 1 + 8), (1024, 512, 256 + 8), (64, 128, 4 * 16 + 4)])
def test_vae_attention_chain(HW, C, tile):
    """The per-sample chain _VaePlan.attn_block builds: pack K (mode 5), pack V transposed (mode 5, T = 1), S = q K^T (conv with a
    device-packed B operand, fp32 A), P = softmax(S / sqrt C) -> bf16 (mode 6), out = P V (conv).  Per element against float64 attention
    that rounds q, K, V and P to bf16 where the kernels do; the accumulation term is the conv bound of fused_cases.py
    (c = ceil(K / 128) + 32 + 8 + 1 roundings on the sum of magnitudes); P's rounding may go either way where its fp32 value is within its
    own uncertainty of a tie.  Tile 256 + 16 + 8: k_conv_lds; 256 + 8: the default LDS-tiled kernel; 68: k_conv_igemm."""
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(HW + C)
    q, k, v = (torch.randn(HW, C, generator=g) * s for s in (1.5, 1.5, 1.0))
    scale = float(int(C) ** -0.5)
    kp = torch.full((lib.sf_conv_packed_elems(HW, C, 1, 1),), 0x7fc0, dtype=torch.int16, device=DEV)
    vp = torch.full((lib.sf_conv_packed_elems(C, HW, 1, 1),), 0x7fc0, dtype=torch.int16, device=DEV)
    s = torch.full((HW, HW), float("nan"), device=DEV)
    pr = torch.full((HW, HW), float("nan"), dtype=torch.bfloat16, device=DEV)
    o = torch.full((HW, C), float("nan"), device=DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ops = [mkop(nc.OP_ELTWISE, 5, p=(kd, None, None, kp), i=(HW, C, C, 0)),
           mkop(nc.OP_ELTWISE, 5, p=(vd, None, None, vp), i=(C, HW, C, 1)),
           mkop(nc.OP_CONV, 1, p=(qd, kp, None, s, None, None), i=(1, 1, HW, C, 1, HW, HW, HW, 0, 1, 1, 1, 0, 1, tile)),
           mkop(nc.OP_ELTWISE, 6, p=(s, None, None, pr), i=(HW, HW), f=(scale,)),
           mkop(nc.OP_CONV, 0, p=(pr, vp, None, o, None, None), i=(1, 1, HW, HW, 1, HW, C, C, 0, 1, 1, 1, 0, 1, tile))]
    assert run(ops) == 0
    q64, k64, v64 = bf(q).double(), bf(k).double(), bf(v).double()
    c1, c2 = math.ceil(C / 128) + 41, math.ceil(HW / 128) + 41
    # stage by stage, each against float64 of the same operation on what the kernel read
    S64, dS = q64 @ k64.t(), c1 * U24 * (q64.abs() @ k64.abs().t())
    Sg = s.cpu()
    assert bool(torch.isfinite(Sg).all())
    rS = float(((Sg.double() - S64).abs() / dS).max())
    P64, dP = nc.softmax_ref64(Sg, scale)
    Pg = pr.cpu()
    nc.check_bf16(f"vae attention ({HW}, {C}) tile {tile}: softmax of the scores as read back", Pg, P64, dP)
    O64, dO = Pg.double() @ v64, c2 * U24 * (Pg.double().abs() @ v64.abs())
    Og = o.cpu()
    assert bool(torch.isfinite(Og).all())
    rO = float(((Og.double() - O64).abs() / dO).max())
    # end to end: the uncertainty of the scores carried through the softmax, either rounding of P inside it
    t = S64 * nc.f32(scale)
    p = torch.softmax(t, 1)
    dt = nc.f32(scale) * dS
    _, dp0 = nc.softmax_ref64((S64).float(), scale)
    dp = dp0 + p * (dt + dt.max(1, keepdim=True).values)
    lo, hi, mid = bf(p - dp).double(), bf(p + dp).double(), bf(p).double()
    want = mid @ v64
    bound = (hi - lo) @ v64.abs() + c2 * U24 * (mid @ v64.abs())
    rE = float(((Og.double() - want).abs() / bound).max())
    amb = float(((hi - lo) > 0).double().mean())
    print(f"margin vae attention ({HW}, {C}) tile {tile}: scores worst err/bound {rS:.3f}; P V of P as read back {rO:.3f}; end to end {rE:.3f} "
          f"(ambiguous share of P {amb:.4f}); rel-L2 {float((Og.double() - want).norm() / want.norm()):.2e}")
    assert rS <= 1 and rO <= 1 and rE <= 1

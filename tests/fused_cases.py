"""Shared cases of the fused UNet kernels (sparsefusion_amd/csrc/fused_kernels.h): the same op descriptors run either on
CPU threads (backend "emu": tests/hostemu, kernel logic without a GPU) or through the C ABI on the GPU (backend "gpu":
sf_plan_run), and are compared with references of the same op (GroupNorm / LayerNorm -> scale/shift -> SiLU -> conv,
external/imagen_pytorch.py:641-662).

The conv cases (run_conv_case) carry two checks:
  * the whole-tensor one: relative L2 < 4e-3 against a plain torch fp32 reference on bf16-rounded operands;
  * the per-element one (conv_reference64 below): a float64 reference that rounds where the kernel rounds, and for EVERY output
    element a bound derived from the roundings of the kernel's path -- which way an operand next to a rounding tie of the operand
    type may legitimately go, fp32 accumulation in any order, the fp32 epilogue adds.  No constant of it is fitted to a kernel's
    output; the measured margins of both backends are in profiles/fused_conv_parity_margins.log."""
import math

import torch
import torch.nn.functional as F

from hostemu import fused
from sparsefusion_amd import _lib

OP_FCONV, OP_SLOTS, OP_GCA = 14, 15, 16
NONE, GN_SELF, GN_SLOTS, LN, ATTN = 0, 1, 2, 3, 4


def bf(x):
    return x.to(torch.bfloat16).float()


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-20))


def slots_of(x, M, C):
    """[M/16][C/16][2] (sum, sum of squares) over 16-pixel x 16-channel blocks of an NHWC [M, C] tensor."""
    t = x.reshape(M // 16, 16, C // 16, 16).permute(0, 2, 1, 3).reshape(M // 16, C // 16, 256)
    return torch.stack([t.sum(-1), (t * t).sum(-1)], -1).contiguous()


def nhwc(x, B, H, W):      # [M, C] -> NCHW
    return x.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def to_rows(x):            # NCHW -> [M, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# The per-element bound.  u = 2^-24 is the unit roundoff of fp32 round-to-nearest; an operation the ISA documents as accurate to
# 1 ulp (v_exp_f32, v_rcp_f32, v_rsq_f32: "CDNA4 ISA", VOP1 transcendental accuracy) is 2 u.  Every term is first order in u.
#
# (a) the staged value  y = ((x - mean) * rstd * gamma + beta) * (scale + 1) + shift,  s = SiLU(y).
#   The kernels evaluate it as x * A + Bv with A = rstd * gamma * (scale + 1) [* scale2] and Bv = (beta - A0 * mean) * (scale + 1) +
#   shift (fused_conv3s.h consume(), fused_kernels.h build_table(), fused_conv4.h), the LayerNorm ones as (x - mean) * rstd * gamma
#   + beta.  x * A and mean * A cancel, so a rounding acts on the magnitude of the TERMS, not of y:
#       M  = ((|x| + |mean|) * rstd * |gamma| + |beta|) * |scale + 1| + |shift|.
#   Roundings on the longest path through the affine (Bv of fused_conv3s.h): gamma * rstd, * mean, beta - ., scale + 1, * (scale + 1),
#   + shift, the final fma, and mean's own double -> float: 8 = N_AFF.
#   rstd = v_rsq((float) var + eps): 2 roundings + 1 ulp = 4 u on its argument, i.e. 2 u on rstd, rounded up to 3 u.
#   The statistics come from fp32 sums; a chain of n additions (an fma counts as one) is off by at most n u sum|terms|.  Longest chains:
#     GroupNorm, sum:          N_SUM = 16  (GN_SELF: <= 8 float4 per thread, 3 levels each pair-wise = NV + 2, then <= 6 shuffle levels, then doubles;
#                                           GN_SLOTS: slot * scale, <= 8 slots per lane (<= 512 slots per group), 6 shuffle levels, then doubles)
#     GroupNorm, sum of squares: N_SQ = 40 (GN_SELF: 4 chained fma per float4 = 32, + 6 shuffle levels; GN_SLOTS: as the sum)
#     LayerNorm (two-pass, 16 float4 per thread): mean 16 + 2 + 5 + the division = N_SUM_LN = 24; sum of (x - mean)^2: 64 fma + 5 levels + the
#                                           subtraction + the division <= N_SQ_LN = 72
#   With r2 = E[x^2] / var (>= 1) and E|x| <= sqrt(E[x^2]):   |d mean| <= N_SUM u sqrt(E[x^2]),   d E[x^2] <= N_SQ u E[x^2],
#     GroupNorm: d var <= d E[x^2] + 2 |mean| |d mean|   ->   d rstd / rstd = d var / (2 var) <= (N_SQ r2 + 2 N_SUM |mean| rstd sqrt(r2)) u / 2 =: R u
#     LayerNorm: the squares are of (x - mean), all terms positive:  d var <= N_SQ_LN u var  ->  R = N_SQ_LN / 2  (d mean enters var in second order)
#   (For GN_SLOTS the reference takes its statistics from the very fp32 slots the kernel is given, in float64, so the producer's own
#   summation error is in neither.)  d mean moves y by rstd |gamma (scale + 1)| |d mean| <= N_SUM u M2 with M2 = sqrt(r2) |gamma (scale + 1)|.
#       d(y) = u * ((N_AFF + 3 + R) * M + N_SUM * M2)  +  rstd |gamma (scale + 1)| * (dx + group mean of dx)
#   dx is the uncertainty of a lazily evaluated source (split-K slabs + bias + residual: groups + 1 additions on sum|terms|; gate: one
#   fma + one add; a GELU in front of the LayerNorm: see (c)); 0 for a plain source.
#   SiLU as the kernels write it, y * v_rcp(1 + v_exp(y * -log2 e)): the product y * log2 e is off by u, which moves the exponential
#   by |y| ln2 log2e u = |y| u; + 2 u (v_exp) + u (the add) + 2 u (v_rcp) + u (the product): s is off by (|y| + 6) u |s| on top of what
#   d(y) does through the function.  That is carried by the LOCAL slope silu'(y) = sig(y) (1 + y (1 - sig(y))), with |silu''| <= 1/2 for the
#   remainder.  (|silu'| <= 1.1 everywhere, but the slope is near 0 where s is small against M, and a small s has a small operand ulp: with the
#   global constant those elements alone decide the ambiguous share, and the median bound / rms of the K = 18432 cases was 1.1e-3 .. 1.7e-3.)
#       d(s) = |silu'(y)| d(y) + d(y)^2 / 4 + (|y| + 6) u |s|.
# (b) the accumulation.  A product of two 16-bit operands is exact in fp32.  A term of the sum is rounded when it is added inside its
#   MFMA (<= 32 additions: K = 32), with every later MFMA of its wave's chain (a split-K op gives each of its S slabs K / S of the sum, and
#   every kernel splits a workgroup's share over >= 4 waves: <= ceil(K / (128 S)) steps), in the K-slice reduction in LDS (<= 8 slices) and
#   in the slab sum (S):  c = ceil(K / (128 S)) + 32 + 8 + S.
# (c) GELU (0.5 v (1 + erff(v / sqrt 2)), OCML erff <= 4 ulp of a value below 1 = 4 u absolute): 0.5 |v| (4 u + u) + 2 u |gelu| + the
#   rounding of v / sqrt 2 through the slope: below 8 u |v|.  Its slope is at most 1.13.
U24 = 2.0 ** -24
N_AFF, N_SUM, N_SQ, N_SUM_LN, N_SQ_LN = 8, 16, 40, 24, 72
AMB_SHARE_MAX, BOUND_MEDIAN_MAX = 0.05, 1e-3        # conditions of the reference alone (asserted): see run_conv_case
# cases left on the whole-tensor norm alone (name -> reason); none: the GELU forms have a derived bound, (c) above
NORM_CHECK_ONLY = {}


def opnd_dtype(backend):
    """The MFMA operand type of the build under test: the emulation is a bf16 build, the GPU library says what it is."""
    return torch.bfloat16 if backend == "emu" else _lib.operand_dtype()


def _rnd(x64, dt):                                     # fp32 -> operand type as the kernels convert, kept in float64
    return x64.float().to(dt).double()


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))


def _conv64(x_rows, w64, B, H, W):                     # [M, C] float64, [Cout, C, k, k] -> [M, Cout]
    return to_rows(F.conv2d(nhwc(x_rows, B, H, W), w64, None, padding=w64.shape[-1] // 2))


def staged_reference64(x, dx, B, HW, norm, G, gamma, beta, ssv, silu, eps, stats=None, pre_gelu=False):
    """float64 value s of the conv's A operand before its rounding to the operand type, and the uncertainty d of the kernel's fp32
    evaluation of it (derivation (a) above).  x, dx: [M, C] float64; stats: per (image, group) float64 (sum, sum of squares) the kernel
    is handed (GN_SLOTS), else they are taken from x."""
    M, C = x.shape
    if norm == NONE:
        y, dy = x, dx
    else:
        if norm == LN:
            if pre_gelu:
                dx = 1.13 * dx + 8 * U24 * x.abs()
                x = _gelu64(x)
            xg, dg = x.view(M, 1, C), dx.view(M, 1, C)
        else:
            xg = x.view(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B * G, 1, -1)        # [image x group][1][HW * Cg]
            dg = dx.view(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B * G, 1, -1)
        n = xg.shape[-1]
        if stats is None:
            s1, s2 = xg.sum(-1, keepdim=True), (xg * xg).sum(-1, keepdim=True)
        else:
            s1, s2 = stats[..., 0].reshape(-1, 1, 1), stats[..., 1].reshape(-1, 1, 1)
        mean, ex2 = s1 / n, s2 / n
        var = (ex2 - mean * mean).clamp(min=0)
        rstd = (var + eps).rsqrt()
        r2 = ex2 / var
        back = (lambda t: t.expand_as(xg).reshape(M, C)) if norm == LN else \
               (lambda t: t.expand_as(xg).reshape(B, G, HW, C // G).permute(0, 2, 1, 3).reshape(M, C))
        mean, rstd, r2, dxm = back(mean), back(rstd), back(r2), back(dg.mean(-1, keepdim=True))
        g64 = gamma.double()
        b64 = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
        if ssv is not None:
            sc = (ssv[:, :C].double() + 1).repeat_interleave(HW, 0)
            sh = ssv[:, C:].double().repeat_interleave(HW, 0)
        else:
            sc, sh = torch.ones(M, C, dtype=torch.float64), torch.zeros(M, C, dtype=torch.float64)
        y = ((x - mean) * rstd * g64 + b64) * sc + sh
        mag = ((x.abs() + mean.abs()) * rstd * g64.abs() + b64.abs()) * sc.abs() + sh.abs()
        slope = rstd * (g64 * sc).abs()
        nsum = N_SUM_LN if norm == LN else N_SUM
        R = N_SQ_LN / 2 if norm == LN else (N_SQ * r2 + 2 * N_SUM * mean.abs() * rstd * r2.sqrt()) / 2
        dy = U24 * ((N_AFF + 3 + R) * mag + nsum * r2.sqrt() * (g64 * sc).abs()) + slope * (dx + dxm)
    if not silu:
        return y, dy
    sg = torch.sigmoid(y)
    s = y * sg
    return s, (sg * (1 + y * (1 - sg))).abs() * dy + dy * dy / 4 + (y.abs() + 6) * U24 * s.abs()


def conv_reference64(s, d, w, dt, B, H, W, S=1):
    """want (before the epilogue adds) and the per-element bound of the conv of the operand-rounded staged value: the rounding-tie
    allowance and fp32 accumulation in any order ((b) above).  Returns want [M, Cout], bound, the ambiguous share of the operand."""
    lo, hi, mid = _rnd(s - d, dt), _rnd(s + d, dt), _rnd(s, dt)
    amb = hi - lo
    w64 = _rnd(w.double(), dt)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    c = math.ceil(K / (128 * S)) + 32 + 8 + S
    want = _conv64(mid, w64, B, H, W)
    ab = _conv64(torch.cat([amb, c * U24 * mid.abs()], 0), w64.abs(), 2 * B, H, W)
    return want, ab[:s.shape[0]] + ab[s.shape[0]:], float((amb > 0).double().mean())


def where_is(idx, Cout, B, H, W, WM, WN, tw):
    """(image, row, column, channel) of flat output element idx and its place in the launch: tile, n-tile, fragment, lane, register
    (D fragment of v_mfma_f32_16x16x32: lane l holds rows 4 (l >> 4) + r, column l & 15)."""
    m, n = divmod(int(idx), Cout)
    b, r, x = m // (H * W), (m % (H * W)) // W, m % W
    TW = tw or W
    TH = max(1, 16 * WM // TW)
    p = (r % TH) * TW + x % TW
    return (f"image {b} row {r} column {x} channel {n}: tile ({r // TH}, {x // TW}) n-tile {n // (16 * WN)} fragment (mi {p // 16}, ni {n // 16 % WN}) "
            f"lane {n % 16 + 16 * (p % 16 // 4)} register {p % 4}")


def check_elements(what, got, want, bound, Cout, B, H, W, WM, WN, tw):
    """|got - want| <= bound for every element: (worst err / bound, None or the report of a failure)."""
    err = (got.double() - want).abs()
    ratio = err / bound.clamp(min=1e-300)
    worst = int(ratio.argmax())
    bad = int((err > bound).sum())
    msg = None if bad == 0 else (f"{what}: {bad} of {err.numel()} elements outside their bound; worst err / bound {float(ratio.view(-1)[worst]):.3g} "
                                 f"(err {float(err.view(-1)[worst]):.3g}) at {where_is(worst, Cout, B, H, W, WM, WN, tw)}")
    return float(ratio.view(-1)[worst]), msg


TIMING_LIB = None          # tools/fconv_phases.py: the instrumented build of unet_fused.hip (libsf_fused_timing.so)


def run_ops(ops, backend):
    if backend == "emu":
        fused.run(ops)
    elif TIMING_LIB is not None:
        for o in ops:
            if TIMING_LIB.sf_fused_op_run(_lib.C.byref(o), _lib.stream_ptr()):
                raise RuntimeError("timing lib: op failed")
        torch.cuda.synchronize()
    else:
        arr = (_lib.SfOp * len(ops))(*ops)
        _lib.check(_lib.lib().sf_plan_run(arr, len(ops), _lib.stream_ptr()), "plan")
        torch.cuda.synchronize()


def run_conv_case(backend, B, H, W, C1, C2, Cout, k, norm, WM, WN, S=1, lazy=0, silu=True, ss=True, accum=False, resid=False,
                  slots=True, pre_gelu=False, ln_bias=False, seed=0, G=8, scale2=2 ** -0.5, tol=4e-3, dbg=None, reps=1, logits=False,
                  out_gelu=False, pair=False, pipe=False, pool=False, general=False, one_image=False, tw=None, keep_pipe=False, name=None):
    """Returns the whole-tensor relative L2 error; `name` labels the margin line the case prints (and selects NORM_CHECK_ONLY).
    tw (r06): run the op on k_conv3s with a tw-pixel-wide tile (W = full-width strips): plain output rows, op field i[19] = tw << 2;
    keep_pipe: the same op with i[19] bit 1 set = the general pipelined kernel."""
    dev = "cpu" if backend == "emu" else "cuda:0"
    d = lambda t: None if t is None else t.to(dev)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    M, HW, C = B * H * W, H * W, C1 + C2
    TR = 16 * WM // W
    # ---- source 1 (possibly lazy) and source 2
    if lazy == 1:
        groups, npad = 3, C1 + 16
        ws = rn(groups, M, npad) * 0.5
        bias1, r1 = rn(C1), rn(M, C1)
        x1 = ws[:, :, :C1].sum(0) + bias1 + r1
        x1_64 = ws[:, :, :C1].double().sum(0) + bias1.double() + r1.double()
        dx1 = (groups + 1) * U24 * (ws[:, :, :C1].double().abs().sum(0) + bias1.double().abs() + r1.double().abs())
        s1 = dict(p=d(torch.full((M, C1), float("nan"))), a=d(ws), b=d(bias1), r=d(r1), mode=1, groups=groups, npad=npad)
    elif lazy == 2:
        hh, gate, r1 = rn(M, C1), torch.sigmoid(rn(B, C1)), rn(M, C1)
        x1 = hh * gate.repeat_interleave(HW, 0) + r1
        x1_64 = hh.double() * gate.double().repeat_interleave(HW, 0) + r1.double()
        dx1 = 2 * U24 * ((hh.double() * gate.double().repeat_interleave(HW, 0)).abs() + r1.double().abs())
        s1 = dict(p=d(torch.full((M, C1), float("nan"))), a=d(hh), b=d(gate), r=d(r1), mode=2, groups=0, npad=0)
    else:
        x1 = rn(M, C1) * 1.5 + 0.3
        x1_64, dx1 = x1.double(), torch.zeros(M, C1, dtype=torch.float64)
        s1 = dict(p=d(x1.clone()), a=None, b=None, r=None, mode=0, groups=0, npad=0)
    x2 = rn(M, C2) if C2 else None
    xc = torch.cat([x1, x2 * scale2], 1) if C2 else x1
    dt = opnd_dtype(backend)
    sc2_32 = float(torch.tensor(scale2, dtype=torch.float32))                  # the op carries scale2 as a float
    eps32 = float(torch.tensor(1e-5, dtype=torch.float32))
    # source 2 as the kernel sees it: without a norm it is ONE fp32 product, rounded to the operand type (bit for bit reproducible); under a
    # norm the scale may be folded into the slope (fused_conv3s.h), which is one of the N_AFF roundings
    x2_64 = ((x2 * torch.tensor(sc2_32)).double() if norm == NONE else x2.double() * sc2_32) if C2 else None
    xc64 = torch.cat([x1_64, x2_64], 1) if C2 else x1_64
    dxc = torch.cat([dx1, torch.zeros(M, C2, dtype=torch.float64)], 1) if C2 else dx1
    # ---- reference
    gamma, beta = rn(C) * 0.5 + 1, rn(C) * 0.2
    ssv = rn(B, 2 * C) * 0.3 if (ss and norm in (GN_SELF, GN_SLOTS)) else None
    if norm in (GN_SELF, GN_SLOTS):
        y = F.group_norm(nhwc(xc, B, H, W), G, gamma, beta, eps=1e-5)
        if ssv is not None:
            y = y * (ssv[:, :C, None, None] + 1) + ssv[:, C:, None, None]
    elif norm == LN:
        u = F.gelu(xc) if pre_gelu else xc
        mean, var = u.mean(1, keepdim=True), u.var(1, unbiased=False, keepdim=True)
        y = nhwc((u - mean) * (var + 1e-5).rsqrt() * gamma + (beta if ln_bias else 0), B, H, W)
    else:
        y = nhwc(xc, B, H, W)
    if silu:
        y = F.silu(y)
    w = rn(Cout, C, k, k) / (C * k * k) ** 0.5
    bias = rn(Cout)
    rd = lambda t: t.to(dt).float()                       # operand rounding of the build under test (bf16, or IEEE half for the _f16 library)
    ref = to_rows(F.conv2d(rd(y), rd(w), None, padding=k // 2))
    # ---- op
    ldc, co_off = (Cout, 0) if (pool or tw is not None) else (Cout + 32, 16)     # epilogue pooling / k_conv3s want the bare conv output
    out0 = rn(M, ldc)
    out = d(out0.clone())
    res = rn(M, ldc) if resid else None
    res_d = d(res)
    wp = d(fused.pack_conv_weights(w, dt))
    wsl = d(torch.full((S, M, (Cout + 15) // 16 * 16), float("nan"))) if S > 1 else None
    slots_out = d(torch.full((M // 16, ldc // 16, 2), float("nan"))) if (slots and S == 1 and Cout % 16 == 0) else None
    sl1 = d(slots_of(x1, M, C1)) if norm == GN_SLOTS else None
    sl2 = d(slots_of(x2, M, C2)) if (norm == GN_SLOTS and C2) else None
    x2_d, bias_d, gamma_d, ssv_d = d(x2), d(bias), d(gamma), d(ssv)
    beta_d = d(beta) if (norm != LN or ln_bias) else None
    n_frags = (Cout + 15) // 16
    wk = rn(Cout) if (logits or pool) else None
    wk_d = d(wk)
    lpart = d(torch.full((S * n_frags, M), float("nan"))) if logits else None
    if pool:          # GlobalContext pooling in the epilogue: w_eff[tap][channel] = sum_n wk[n] * W[n][channel][tap], k-step order, bf16
        assert pipe and not logits and k == 3
        weff = torch.einsum("n,ncyx->yxc", wk, rd(w)).reshape(-1).to(dt).contiguous()
        wk_d = d(weff)
        lpart = d(torch.full((M // 16 * Cout + M // 16 * 2,), float("nan")))
    op = fused.mkop(OP_FCONV, (1 if silu else 0) | (2 if pre_gelu else 0) | (4 if accum else 0) | (8 if out_gelu else 0) | (32 if pipe else 0)
                    | (64 if pool else 0) | (128 if general else 0),     # 128: keep the general kernel (r05: k_conv4_gn takes the 4x4 geometry otherwise)
                    p=(s1["p"], s1["a"], s1["b"], s1["r"], sl1, x2_d, sl2, wp, bias_d, out, res_d, wsl, slots_out, gamma_d, beta_d, ssv_d, dbg, wk_d, lpart),
                    i=(B, H, W, C1, C2, Cout, ldc, co_off, k, s1["mode"], s1["groups"], s1["npad"], norm, G, TR, WM, WN, S, 2 * C)
                    + ((1,) if one_image else ((((0 if tw == W else tw) << 2) | (2 if keep_pipe else 0),) if tw is not None else ())),      # i[19] bit 0: one image per workgroup (k_conv4_gn) where k_conv4_gn_mb would take the op; bit 1 / bits 2..: k_conv3s
                    f=(1e-5, 1.0, scale2))
    ops = [op]
    # ---- float64 reference with the kernel's rounding points, and its per-element bound
    stats = None
    if norm == GN_SLOTS:               # the statistics the kernel is handed: its fp32 producer slots (source 2: scaled by scale2, scale2^2)
        assert (C // G) % 16 == 0
        sl_all = sl1.cpu().double() if not C2 else torch.cat([sl1.cpu().double(), sl2.cpu().double() * torch.tensor([sc2_32, sc2_32 * sc2_32], dtype=torch.float64)], 1)
        stats = sl_all.view(B, HW // 16, G, C // G // 16, 2).sum((1, 3))
    s64, ds64 = staged_reference64(xc64, dxc, B, HW, norm, G, gamma, beta if (norm != LN or ln_bias) else None, ssv, silu, eps32, stats, pre_gelu)
    conv64, bound, amb_share = conv_reference64(s64, ds64, w, dt, B, H, W, S)
    if pair:          # conv1 || res_conv in one launch (k_conv_fused_pair): a 1x1 conv of the RAW concat next to the normalised 3x3 one
        w2 = rn(Cout, C, 1, 1) / C ** 0.5
        bias2 = rn(Cout)
        ref2 = to_rows(F.conv2d(rd(nhwc(xc, B, H, W)), rd(w2), None)) + bias2
        xr64 = torch.cat([x1_64, (x2 * torch.tensor(sc2_32)).double()], 1) if C2 else x1_64       # raw operand: reproducible bit for bit unless lazy
        conv2_64, bound2, _ = conv_reference64(xr64, dxc, w2, dt, B, H, W)
        want2_64 = conv2_64 + bias2.double()
        bound2 = bound2 + 2 * U24 * (conv2_64.abs() + bias2.double().abs())
        out2 = d(torch.full((M, Cout), float("nan")))
        wp2, bias2_d = d(fused.pack_conv_weights(w2, dt)), d(bias2)
        op.flags |= 16
        ops.append(fused.mkop(OP_FCONV, 0,
                              p=(s1["p"] if not lazy else None, s1["a"], s1["b"], s1["r"], None, x2_d, None, wp2, bias2_d, out2, None, None, None,
                                 None, None, None, None, None, None),
                              i=(B, H, W, C1, C2, Cout, Cout, 0, 1, s1["mode"], s1["groups"], s1["npad"], NONE, G, TR, WM, WN, 1, 0),
                              f=(1e-5, 1.0, scale2)))
    run_ops(ops, backend)
    if pair:
        e2 = rel(out2.cpu(), ref2)
        assert e2 < tol, f"paired res_conv mismatch rel {e2}"
    if reps > 1:                                         # timing aid (tools/fconv_phases.py): the output is re-written, not checked again
        import time
        t0 = time.time()
        run_ops(ops * reps, backend)
        return (time.time() - t0) / reps
    out = out.cpu()
    if S > 1:
        got = wsl.cpu()[:, :, :Cout].sum(0)
        want = ref
    else:
        got = out[:, co_off:co_off + Cout]
        want = ref + bias
        if resid:
            want = want + res[:, co_off:co_off + Cout]
        if accum:
            want = want + out0[:, co_off:co_off + Cout]
        if out_gelu:
            want = F.gelu(want)
        # columns outside [co_off, co_off + Cout) are untouched
        assert torch.equal(out[:, :co_off], out0[:, :co_off]) and torch.equal(out[:, co_off + Cout:], out0[:, co_off + Cout:])
    assert torch.isfinite(got).all()
    e = rel(got, want)
    # the float64 counterpart of `want` and the epilogue's share of the bound: every fp32 add rounds its own result, which is at most the sum
    # of the magnitudes of what has been added; at most two adds follow the K-slice reduction in any case (bias, and residual or accumulate)
    want64, parts = conv64, conv64.abs()
    if S == 1:
        for t in (bias, res[:, co_off:co_off + Cout] if resid else None, out0[:, co_off:co_off + Cout] if accum else None):
            if t is not None:
                want64, parts = want64 + t.double(), parts + t.double().abs()
    bound = bound + 2 * U24 * parts
    if out_gelu:                                         # derivation (c): slope <= 1.13, evaluation error < 8 u |v|
        bound = 1.13 * bound + 8 * U24 * want64.abs()
        want64 = _gelu64(want64)
        bound = bound + U24 * want64.abs()
    rms = float(want64.pow(2).mean().sqrt())
    med = float(bound.median()) / rms
    worst, fails = float("nan"), []
    if name not in NORM_CHECK_ONLY:
        worst, msg = check_elements("conv", got, want64, bound, Cout, B, H, W, WM, WN, tw)
        fails.append(msg)
        if pair:
            w2_, msg = check_elements("paired res_conv", out2.cpu(), want2_64, bound2, Cout, B, H, W, WM, WN, tw)
            worst = max(worst, w2_)
            fails.append(msg)
    print(f"margin {backend} {name}: rel-L2 {e:.2e} worst err/bound {worst:.3f} ambiguous {amb_share:.4f} median bound/rms {med:.2e}")
    # conditions on the reference alone: the allowance cannot grow quietly
    assert amb_share <= AMB_SHARE_MAX, f"ambiguous share {amb_share:.3g} of the operand: change the case's seed"
    assert norm not in (GN_SELF, GN_SLOTS) or med <= BOUND_MEDIAN_MAX, f"median bound / rms {med:.3g}"
    assert not any(fails), "; ".join(m for m in fails if m)
    assert e < tol, f"conv mismatch rel {e}"
    if lazy:
        assert torch.allclose(s1["p"].cpu(), x1, atol=1e-5), "lazy source not materialised correctly"
    if logits:                                           # partial context logits: per-pixel sums equal value . wk (bias excluded when sliced)
        assert not (accum or resid)                      # the GlobalContext input is the bare conv output (bias is pixel-constant)
        val = got if S > 1 else out[:, co_off:co_off + Cout] - bias
        assert torch.allclose(lpart.cpu().sum(0), val @ wk, rtol=1e-3, atol=2e-3), "context logits wrong"
    if pool:                                             # merged over the 16-pixel chunks of an image = softmax(out . wk) pooling of out
        buf = lpart.cpu()
        part, ms = buf[:M // 16 * Cout].view(B, HW // 16, Cout), buf[M // 16 * Cout:].view(B, HW // 16, 2)
        assert torch.isfinite(buf).all()
        mx = ms[..., 0].max(1, keepdim=True).values
        wj = (ms[..., 0] - mx).exp()
        pooled = (wj[..., None] * part).sum(1) / (wj * ms[..., 1]).sum(1, keepdim=True)
        val = out[:, :Cout]
        lg = ((val - bias) @ wk).view(B, HW)
        want_pool = torch.einsum("bp,bpc->bc", torch.softmax(lg, 1), val.view(B, HW, Cout))
        ep = rel(pooled, want_pool)
        assert ep < 2e-2, f"epilogue pooling mismatch rel {ep}"
    if slots_out is not None:
        sl = slots_of(out[:, co_off:co_off + Cout].contiguous(), M, Cout)
        got_sl = slots_out.cpu()[:, co_off // 16:co_off // 16 + Cout // 16]
        if tw is not None and tw != W:                   # 2-D tiles: a fragment holds a 16-pixel patch, not 16 consecutive pixels; consumers sum per image
            sl, got_sl = sl.view(B, HW // 16, Cout // 16, 2).sum(1), got_sl.reshape(B, HW // 16, Cout // 16, 2).sum(1)
        assert torch.allclose(got_sl, sl, rtol=1e-4, atol=2e-3 * (1 if tw is None or tw == W else HW // 16) ** 0.5), "output slots wrong"
        # derived: float64 slot sums of the kernel's OWN output; a slot is the sum of 256 fp32 values (and of their fma'd squares) in some
        # order: at most 256 roundings on sum |v| / sum v^2.  (Asserted next to the allclose above until it has held on the GPU.)
        o64 = out[:, co_off:co_off + Cout].double().contiguous()
        sl64, sla = slots_of(o64, M, Cout), slots_of(o64.abs(), M, Cout)
        g64 = slots_out.cpu()[:, co_off // 16:co_off // 16 + Cout // 16].double()
        if tw is not None and tw != W:
            sl64, sla, g64 = (t.reshape(B, HW // 16, Cout // 16, 2).sum(1) for t in (sl64, sla, g64))
        sl_bound = 256 * U24 * torch.stack([sla[..., 0], sl64[..., 1]], -1)
        nbad = int(((g64 - sl64).abs() > sl_bound).sum())
        assert nbad == 0, f"output slots: {nbad} outside 256 fp32 roundings, worst err / bound {float(((g64 - sl64).abs() / sl_bound).max()):.3g}"
    return e


def run_slots_case(backend):
    dev = "cpu" if backend == "emu" else "cuda:0"
    g = torch.Generator().manual_seed(9)
    M, C, HW = 64, 48, 32
    h, gate, res = torch.randn(M, C, generator=g), torch.rand(2, C, generator=g), torch.randn(M, C, generator=g)
    hd, gd, rd = h.to(dev), gate.to(dev), res.to(dev)
    out, sl = torch.zeros(M, C, device=dev), torch.zeros(M // 16, C // 16, 2, device=dev)
    run_ops([fused.mkop(OP_SLOTS, p=(hd, gd, rd, out, sl), i=(M, C, HW))], backend)
    x = h * gate.repeat_interleave(HW, 0) + res
    assert torch.allclose(out.cpu(), x, atol=1e-6) and torch.allclose(sl.cpu(), slots_of(x, M, C), rtol=1e-5, atol=1e-4)
    # split-K source: x = bias + sum of slabs, materialised into `out3`
    groups, npad = 3, C + 16
    ws = torch.randn(groups, M, npad, generator=g)
    bias = torch.randn(C, generator=g)
    x3 = ws[:, :, :C].sum(0) + bias
    out3, sl3 = torch.full((M, C), float("nan"), device=dev), torch.zeros_like(sl)
    wsd, bd = ws.to(dev), bias.to(dev)
    run_ops([fused.mkop(OP_SLOTS, p=(None, None, None, out3, sl3, wsd, bd), i=(M, C, HW, groups, npad))], backend)
    assert torch.allclose(out3.cpu(), x3, atol=1e-5) and torch.allclose(sl3.cpu(), slots_of(x3, M, C), rtol=1e-5, atol=1e-4)
    sl2, xd = torch.zeros_like(sl), x.to(dev)
    run_ops([fused.mkop(OP_SLOTS, p=(xd, None, None, None, sl2), i=(M, C, HW))], backend)
    assert torch.allclose(sl2.cpu(), slots_of(x, M, C), rtol=1e-5, atol=1e-4)


def run_gca_case(backend, B, H, C, lazy=False, seed=0, epilogue_chunks=False, rc=None):
    """k_gca_pool -> k_gca_net0 -> k_gca_gate against GlobalContext + gated residual (imagen_pytorch.py:916-941, :727-729).
    rc = (C1, C2): the residual is the block's res_conv -- a 1x1 conv of the raw concat(x, skip * 2^-1/2) -- computed by an
    un-normalised fconv op that shares the pooling launch (k_gca_pool_rc, r04: flag 16 on the fconv, the pooling op right behind it)."""
    dev = "cpu" if backend == "emu" else "cuda:0"
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    HW, M, HID = H * H, B * H * H, max(3, C // 2)
    h2, res, wk = rn(M, C), rn(M, C), rn(C) * 0.3
    W0, b0, W2, b2 = rn(HID, C) / C ** 0.5, rn(HID) * 0.1, rn(C, HID) / HID ** 0.5, rn(C) * 0.1
    rc_op = None
    if rc is not None:
        assert not epilogue_chunks and H == 4
        C1, C2 = rc
        xa, xb = rn(M, C1) * 1.5 + 0.3, (rn(M, C2) if C2 else None)
        xc = torch.cat([xa, xb * 2 ** -0.5], 1) if C2 else xa
        w_rc, b_rc = rn(C, C1 + C2, 1, 1) / (C1 + C2) ** 0.5, rn(C)
        res = to_rows(F.conv2d(bf(nhwc(xc, B, H, H)), bf(w_rc), None)) + b_rc
    sm = torch.softmax((h2 @ wk).view(B, HW), 1)
    pooled = (sm[:, :, None] * h2.view(B, HW, C)).sum(1)
    hid = F.silu(pooled @ bf(W0).t() + b0)
    gate = torch.sigmoid(hid @ bf(W2).t() + b2)
    want = h2 * gate.repeat_interleave(HW, 0) + res
    nparts = C // 16
    lpart = (h2 * wk).view(M, nparts, 16).sum(-1).t().contiguous() + 3.0       # a per-pixel-constant shift must not matter
    chunks = min(8, HW // 16)
    CH = HW // chunks
    Kp, Kp2 = (C + 7) // 8 * 8, (HID + 7) // 8 * 8
    dv = lambda t: t.to(dev)
    if lazy:
        groups, npad = 3, C + 16
        ws = rn(groups, M, npad)
        bias = rn(C)
        ws[0, :, :C] = h2 - ws[1:, :, :C].sum(0) - bias
        h2_d, ws_d, bias_d = dv(torch.full((M, C), float("nan"))), dv(ws), dv(bias)
    else:
        groups = npad = 0
        h2_d, ws_d, bias_d = dv(h2), None, None
    lp_d, res_d = dv(lpart), dv(res)
    if rc is not None:
        res_d = dv(torch.full((M, C), float("nan")))          # written by the res_conv half of the shared launch
        xa_d, xb_d, wrc_d, brc_d = dv(xa), (dv(xb) if C2 else None), dv(fused.pack_conv_weights(w_rc)), dv(b_rc)      # (kept alive: ops hold raw pointers)
        rc_op = fused.mkop(OP_FCONV, 16,
                           p=(xa_d, None, None, None, None, xb_d, None, wrc_d, brc_d, res_d,
                              None, None, None, None, None, None, None, None, None),
                           i=(B, H, H, C1, C2, C, C, 0, 1, 0, 0, 0, NONE, 8, 4, 1, 1, 1, 0), f=(1e-5, 1.0, 2 ** -0.5))
    part_pool, part_ms = torch.zeros(B * chunks, C, device=dev), torch.zeros(B * chunks, 2, device=dev)
    W0p = dv(F.pad(W0, (0, Kp - C)).to(torch.bfloat16).contiguous())
    W2p = dv(F.pad(W2, (0, Kp2 - HID)).to(torch.bfloat16).contiguous())
    b0_d, b2_d = dv(b0), dv(b2)
    hid_d, out = torch.zeros(B, HID, device=dev), torch.zeros(M, C, device=dev)
    slots = torch.zeros(M // 16, C // 16, 2, device=dev)
    head = ([rc_op] if rc_op is not None else []) + [
         fused.mkop(OP_GCA, 1, p=(h2_d, ws_d, bias_d, lp_d, part_pool, part_ms), i=(M, C, HW, CH, chunks, nparts, groups, npad)),
         fused.mkop(OP_GCA, 2, p=(part_pool, part_ms, W0p, b0_d, hid_d), i=(B, C, Kp, HID, chunks))]
    if epilogue_chunks:            # the pooled 16-pixel fragments as the producing conv's epilogue leaves them (fused_pipe.h POOL):
        assert not lazy            # HW / 16 chunks per image, net0 merges up to 64 of them
        chunks = HW // 16
        lg = (h2 @ wk).view(B * chunks, 16)
        mj = lg.max(1, keepdim=True).values
        e = (lg - mj).exp()
        part_pool = dv(torch.einsum("jp,jpc->jc", e, h2.view(B * chunks, 16, C)).contiguous())
        part_ms = dv(torch.cat([mj, e.sum(1, keepdim=True)], 1).contiguous())
        head = [fused.mkop(OP_GCA, 2, p=(part_pool, part_ms, W0p, b0_d, hid_d), i=(B, C, Kp, HID, chunks))]
    ops = head + [
           fused.mkop(OP_GCA, 3, p=(h2_d, res_d, hid_d, W2p, b2_d, out, slots), i=(M, C, HW, HID, Kp2))]
    run_ops(ops, backend)
    assert torch.allclose(hid_d.cpu(), hid, rtol=2e-4, atol=2e-5), "hidden vector wrong"
    if rc is not None:
        assert rel(res_d.cpu(), res) < 4e-3, "res_conv beside the pooling launch wrong"
        want = h2 * gate.repeat_interleave(HW, 0) + res_d.cpu()
    assert torch.allclose(out.cpu(), want, rtol=2e-4, atol=2e-4), "gated residual wrong"
    assert torch.allclose(slots.cpu(), slots_of(want, M, C), rtol=1e-4, atol=2e-3)
    if lazy:
        assert torch.allclose(h2_d.cpu(), h2, atol=1e-5)


def run_attn_case(backend, B=2, cross=False, context=True, Cout=48, seed=0, tol=4e-3, dbg=None, reps=1, WN=1, general=False):
    """k_conv_fused<.., FNORM_ATTN>: the 16-token attention core (8 heads x 64, keys = [context tokens,] null k/v, the tokens' one
    shared k/v head -- or, cross-attention, null + 2 per-head time tokens; imagen_pytorch.py:480-566, :731-805) as the prologue of
    its output projection, against softmax(q k^T scale) v -> bf16 -> linear in torch."""
    dev = "cpu" if backend == "emu" else "cuda:0"
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    heads, dh, inner = 8, 64, 512
    scale = dh ** -0.5
    nq = inner if cross else inner + 2 * dh
    qkv = rn(B * 16, nq) * 1.3
    null_kv = rn(2, dh)
    q = qkv[:, :inner].view(B, 16, heads, dh)
    if cross:                                            # time block row per batch: [.. | k (2 tokens x 8 heads x 64) | v (same)]
        st = 3000
        tb = rn(B, st)
        off = 700
        kt = tb[:, off:off + 2 * inner].view(B, 2, heads, dh)
        vt = tb[:, off + 2 * inner:off + 4 * inner].view(B, 2, heads, dh)
        k = torch.cat([null_kv[0].expand(B, 1, heads, dh), kt], 1)                      # [B, 3, heads, dh]
        v = torch.cat([null_kv[1].expand(B, 1, heads, dh), vt], 1)
        tb_d, nk_d = tb.to(dev), null_kv.reshape(-1).contiguous().to(dev)
        # layout of the plan: k of token t, head h at off + t * (2 * inner) ... the plan's own strides: row = 2 * inner, head = dh, v = k + inner
        kt2 = torch.stack([kt, vt], 2).reshape(B, 2, 2 * inner)                          # [B, token, (k heads | v heads)]
        tb2 = tb.clone()
        tb2[:, off:off + 4 * inner] = kt2.reshape(B, -1)
        tb_d = tb2.to(dev)
        segs = [(nk_d.data_ptr(), nk_d.data_ptr() + dh * 4, 1, 0, 0, 0),
                (tb_d.data_ptr() + off * 4, tb_d.data_ptr() + (off + inner) * 4, 2, 2 * inner, st, dh)]
    else:
        ks = qkv[:, inner:inner + dh].view(B, 16, 1, dh).expand(B, 16, heads, dh)
        vs = qkv[:, inner + dh:].view(B, 16, 1, dh).expand(B, 16, heads, dh)
        parts_k, parts_v, segs = [], [], []
        nk_d = null_kv.reshape(-1).contiguous().to(dev)
        if context:
            st, off = 1000, 300
            tb = rn(B, st)
            ck = tb[:, off:off + 4 * dh].view(B, 2, 2, dh)                               # token t: [k | v]
            parts_k.append(ck[:, :, 0].view(B, 2, 1, dh).expand(B, 2, heads, dh))
            parts_v.append(ck[:, :, 1].view(B, 2, 1, dh).expand(B, 2, heads, dh))
            tb_d = tb.to(dev)
            segs.append((tb_d.data_ptr() + off * 4, tb_d.data_ptr() + (off + dh) * 4, 2, 2 * dh, st, 0))
        parts_k += [null_kv[0].expand(B, 1, heads, dh), ks]
        parts_v += [null_kv[1].expand(B, 1, heads, dh), vs]
        k, v = torch.cat(parts_k, 1), torch.cat(parts_v, 1)
    qkv_d = qkv.to(dev)
    if not cross:
        kp = qkv_d.data_ptr() + inner * 4
        segs += [(nk_d.data_ptr(), nk_d.data_ptr() + dh * 4, 1, 0, 0, 0), (kp, kp + dh * 4, 16, nq, 16 * nq, 0)]
    sim = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    att = torch.einsum("bhij,bjhd->bihd", torch.softmax(sim, -1), v).reshape(B * 16, inner)
    w = rn(Cout, inner, 1, 1) / inner ** 0.5
    bias, res = rn(Cout), rn(B * 16, Cout)
    want = bf(att) @ bf(w.view(Cout, inner)).t() + bias + res
    out = torch.full((B * 16, Cout), float("nan")).to(dev)
    wp, bias_d, res_d = fused.pack_conv_weights(w).to(dev), bias.to(dev), res.to(dev)
    segs = segs + [(0, 0, 0, 0, 0, 0)] * (3 - len(segs))
    op = fused.mkop(OP_FCONV, 128 if general else 0,      # 128: keep the general kernel (r06: k_lin4_attn takes the op otherwise)
                    p=(qkv_d, None, None, None, None, None, None, wp, bias_d, out, res_d, None, None, None, None, None, dbg, None, None) + tuple(sg[0] for sg in segs),
                    i=(B, 4, 4, inner, 0, Cout, Cout, 0, 1, 0, 0, 0, ATTN, 8, 4, 1, WN, 1, 0, nq) + tuple(x for sg in segs for x in sg[2:]),
                    f=(1e-5, 1.0, 1.0) + tuple((sg[1] - sg[0]) // 4 for sg in segs) + (scale,))
    run_ops([op], backend)
    if reps > 1:
        import time
        t0 = time.time()
        run_ops([op] * reps, backend)
        return (time.time() - t0) / reps
    e = rel(out.cpu(), want)
    assert torch.isfinite(out.cpu()).all() and e < tol, f"attention + projection mismatch rel {e}"
    return e


ATTN_CASES = {"self_context": dict(B=2, cross=False, context=True, seed=61), "self_plain": dict(B=1, cross=False, context=False, seed=62),
              "cross_time_tokens": dict(B=2, cross=True, seed=63, Cout=64),
              "self_context_wn2": dict(B=2, cross=False, context=True, seed=68, Cout=64, WN=2),      # the B >= 8 tile of the output projection
              # r06: the cases above run on k_lin4_attn (csrc/fused_conv4.h); op flag 128 keeps k_conv_fused<.., FNORM_ATTN>
              "self_context_on_the_general_kernel": dict(B=2, cross=False, context=True, seed=61, general=True),
              "cross_time_tokens_on_the_general_kernel": dict(B=2, cross=True, seed=63, Cout=64, general=True),
              "self_plain_ragged_cout": dict(B=3, cross=False, context=False, seed=69, Cout=40)}

GCA_CASES = {"4x4_lazy": dict(B=2, H=4, C=128, lazy=True),
             "4x4_lazy_res_conv_beside_pool": dict(B=2, H=4, C=128, lazy=True, seed=21, rc=(96, 64)),
             "4x4_res_conv_beside_pool_no_skip": dict(B=1, H=4, C=64, seed=22, rc=(128, 0)), "8x8": dict(B=1, H=8, C=64, seed=1), "16x16": dict(B=1, H=16, C=64, seed=2),
             "8x8_hid128_gate_t": dict(B=2, H=8, C=256, seed=31),
             "32x32_c256_64_chunks_net0_t": dict(B=1, H=32, C=256, seed=32, epilogue_chunks=True),      # k_gca_net0_t<256, 64>
             "16x16_c512_16_chunks_net0_t": dict(B=1, H=16, C=512, seed=33, epilogue_chunks=True),      # k_gca_net0_t<512, 16>, k_gca_gate_t<256>       # r05: HID = 128 | 256 | 512 run k_gca_gate_t (compile-time hidden width)
             "8x8_c192_b2": dict(B=2, H=8, C=192, seed=8),
             "32x32_epilogue_chunks": dict(B=2, H=32, C=64, seed=11, epilogue_chunks=True),
             "16x16_epilogue_chunks": dict(B=1, H=16, C=320, seed=12, epilogue_chunks=True),
             "8x8_epilogue_chunks": dict(B=2, H=8, C=128, seed=13, epilogue_chunks=True)}
GCA_CASES_FULL = {"unet_32x32_epilogue_chunks": dict(B=1, H=32, C=256, seed=14, epilogue_chunks=True),
                  "unet_b4_16x16_epilogue_chunks": dict(B=4, H=16, C=512, seed=15, epilogue_chunks=True),
                  "unet_4x4": dict(B=1, H=4, C=1024, lazy=True, seed=3),
                  "unet_4x4_res_conv_beside_pool": dict(B=1, H=4, C=1024, lazy=True, seed=23, rc=(1024, 1024)),
                  "unet_b4_4x4_res_conv_beside_pool": dict(B=4, H=4, C=1024, lazy=True, seed=24, rc=(1024, 1024)), "unet_8x8": dict(B=1, H=8, C=1024, seed=4),
                  "unet_32x32": dict(B=1, H=32, C=256, seed=5), "unet_b4_16x16": dict(B=4, H=16, C=512, seed=6)}


# name -> kwargs of run_conv_case; small enough for the CPU-thread emulator, and every kernel path is in here
CONV_CASES = {
    # the 4x4 level: whole image per tile, input-channel slices, lazy split-K source, partial slabs out
    "gn_self_sliced_lazy_splitk_4x4": dict(B=2, H=4, W=4, C1=64, C2=0, Cout=48, k=3, norm=GN_SELF, WM=1, WN=1, S=2, lazy=1, logits=True),
    # 12 channels per group (not a power of two), 24 channel chunks per pixel (512 threads % 24 != 0): the fixed-order fallback
    # of the GN_SELF statistics (r02: LDS float atomics, order dependent)
    "gn_self_odd_groups_fallback_4x4": dict(B=2, H=4, W=4, C1=96, C2=0, Cout=32, k=3, norm=GN_SELF, WM=1, WN=1, seed=41),
    "gn_self_concat_gate_lazy_4x4": dict(B=1, H=4, W=4, C1=64, C2=64, Cout=32, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=2, seed=1),
    # r05: the geometry k_conv4_gn is written for (csrc/fused_conv4.h: 4 slices of two whole groups each, Cs = 256 | 512), every lazy
    # mode, with and without scale / shift and SiLU, partial context logits, two images; `general=True` = the same op on k_conv_fused
    "conv4_gn_lazy_splitk_1024": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=32, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=71, logits=True),
    "conv4_gn_concat_gate_2048": dict(B=1, H=4, W=4, C1=1024, C2=1024, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=2, seed=72),
    "conv4_gn_plain_1024_b2": dict(B=2, H=4, W=4, C1=1024, C2=0, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, ss=False, silu=False, seed=73),
    "conv4_gn_concat_lazy_2048": dict(B=1, H=4, W=4, C1=1024, C2=1024, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=74, logits=True),
    # r05: B >= 2 in that geometry runs k_conv4_gn_mb -- NB = 2 | 4 images per workgroup share its weight slice (B % 4 == 0 at Cs = 256: 4, other
    # even B: 2; Cs = 512: 2); every lazy mode (a split-K element's six loads bound how many images' gathers fly together: 2 at Cs = 256, 1 at
    # Cs = 512), several image groups per (slice, n-tile), logits; `one_image=True` = the same op on k_conv4_gn
    "conv4_mb_lazy_splitk_1024_b4": dict(B=4, H=4, W=4, C1=1024, C2=0, Cout=32, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=75, logits=True),
    "conv4_mb_gate_1024_b8": dict(B=8, H=4, W=4, C1=1024, C2=0, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=2, seed=76),
    "conv4_mb_lazy_splitk_1024_b6": dict(B=6, H=4, W=4, C1=1024, C2=0, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=77, logits=True),
    "conv4_mb_concat_lazy_2048_b2": dict(B=2, H=4, W=4, C1=1024, C2=1024, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=78, logits=True),
    "conv4_mb_concat_gate_2048_b4": dict(B=4, H=4, W=4, C1=1024, C2=1024, Cout=32, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=2, seed=79),
    "conv4_mb_concat_plain_2048_b2": dict(B=2, H=4, W=4, C1=1024, C2=1024, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, seed=80, ss=False),
    "conv4_mb_concat_lazy_512_512_b4": dict(B=4, H=4, W=4, C1=512, C2=512, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=81),
    "conv4_one_image_per_workgroup_b4": dict(B=4, H=4, W=4, C1=1024, C2=0, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=75, one_image=True),
    # r06: the same geometry without a norm (k_conv4_gn<64, 0, false>): the merged 3x3 + 1x1 conv of the last Downsample at B = 1
    "conv4_no_norm_plain_1024": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=32, k=3, norm=NONE, WM=1, WN=1, S=4, silu=False, ss=False, slots=False, seed=145),
    "conv4_geometry_on_the_general_kernel": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=16, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=71, general=True),
    # 8x8 level: 2-row tiles with halo rows from neighbouring tiles, statistics from producer slots, final epilogue + slots
    "gn_slots_concat_8x8": dict(B=1, H=8, W=8, C1=128, C2=128, Cout=32, k=3, norm=GN_SLOTS, WM=1, WN=1, resid=True, seed=2),
    # 32-pixel rows (WM = 2), 2 n-fragments per tile, accumulate mode
    "gn_slots_wide_rows_wm2_wn2": dict(B=2, H=4, W=32, C1=128, C2=0, Cout=64, k=3, norm=GN_SLOTS, WM=2, WN=2, accum=True, seed=3),
    # XCD-aware tile order (8 n-tiles)
    "gn_slots_xcd_map_16x16": dict(B=1, H=16, W=16, C1=128, C2=0, Cout=128, k=3, norm=GN_SLOTS, WM=1, WN=1, ss=False, seed=4, logits=True),
    "raw_1x1_concat_res_conv": dict(B=1, H=8, W=8, C1=64, C2=32, Cout=40, k=1, norm=NONE, WM=1, WN=1, silu=False, slots=False, seed=5),
    # conv1 || res_conv pairs (one launch): slot statistics at 8x8, and the 4x4 level with a lazy split-K source read by both halves
    "pair_gn_slots_concat_8x8": dict(B=1, H=8, W=8, C1=64, C2=64, Cout=32, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=21, pair=True),
    "pair_gn_self_lazy_splitk_4x4": dict(B=2, H=4, W=4, C1=64, C2=64, Cout=48, k=3, norm=GN_SELF, WM=1, WN=1, S=2, lazy=1, seed=22, pair=True),
    "pair_gn_slots_wm2_wn2": dict(B=1, H=2, W=32, C1=128, C2=0, Cout=64, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=23, pair=True),
    # pipelined kernel (k_conv_fused_pipe): 8x8 with halo rows and a concat that changes source inside a chunk's thread range,
    # 16-pixel rows with 2 n-fragments + logits, 32-pixel rows, accumulate + residual
    "pipe_gn_slots_concat_8x8": dict(B=1, H=8, W=8, C1=128, C2=128, Cout=32, k=3, norm=GN_SLOTS, WM=1, WN=1, resid=True, seed=31, pipe=True),
    "pipe_gn_slots_16x16_wn2": dict(B=1, H=16, W=16, C1=256, C2=128, Cout=64, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=32, pipe=True, logits=True),
    "pipe_gn_slots_wm2_wn2_accum": dict(B=2, H=4, W=32, C1=128, C2=0, Cout=64, k=3, norm=GN_SLOTS, WM=2, WN=2, accum=True, seed=33, pipe=True),
    "pipe_pair_gn_slots_concat_8x8": dict(B=1, H=8, W=8, C1=128, C2=128, Cout=32, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=38, pipe=True, pair=True),
    # GlobalContext pooling in the conv's epilogue (context logits from the conv's own input through w_eff)
    "pipe_pool_8x8": dict(B=2, H=8, W=8, C1=128, C2=0, Cout=64, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=54, pipe=True, pool=True),
    "pipe_pool_16x16_wn2": dict(B=1, H=16, W=16, C1=256, C2=0, Cout=64, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=55, pipe=True, pool=True),
    "pipe_pool_16x16_tr2": dict(B=2, H=16, W=16, C1=128, C2=0, Cout=96, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=56, pipe=True, pool=True),
    "pipe_pool_wide_rows_wm4": dict(B=2, H=4, W=32, C1=128, C2=0, Cout=64, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=57, pipe=True, pool=True),
    # 32-pixel tiles of the 16x16 / 8x8 maps (the B >= 4 geometry): two row pairs / four rows per workgroup
    "pipe_gn_slots_16x16_tr2_wn2": dict(B=2, H=16, W=16, C1=256, C2=128, Cout=64, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=42, pipe=True, logits=True),
    "pipe_gn_slots_wide_rows_wm4_wn2": dict(B=2, H=4, W=32, C1=128, C2=128, Cout=64, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=47, pipe=True, logits=True),
    "pipe_pair_gn_slots_wide_rows_wm4": dict(B=1, H=4, W=32, C1=128, C2=0, Cout=64, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=48, pipe=True, pair=True),
    "gn_slots_wide_rows_wm4_wn1": dict(B=1, H=4, W=32, C1=128, C2=0, Cout=48, k=3, norm=GN_SLOTS, WM=4, WN=1, seed=49),
    "pipe_gn_slots_8x8_wn2": dict(B=2, H=8, W=8, C1=128, C2=128, Cout=64, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=46, pipe=True),
    "pipe_gn_slots_8x8_tr4_resid": dict(B=2, H=8, W=8, C1=128, C2=128, Cout=48, k=3, norm=GN_SLOTS, WM=2, WN=1, resid=True, seed=43, pipe=True),
    "pipe_pair_gn_slots_16x16_tr2": dict(B=2, H=16, W=16, C1=128, C2=128, Cout=64, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=44, pipe=True, pair=True),
    "raw_1x1_res_conv_8x8_tr4": dict(B=2, H=8, W=8, C1=64, C2=64, Cout=32, k=1, norm=NONE, WM=2, WN=2, silu=False, slots=False, seed=45),
    # r05: the shapes k_lin4_ln takes (csrc/fused_conv4.h: plain source of 1024 | 2048 channels on the 16-token map): ff1 with its GELU
    # epilogue, ff2 with residual and two n-fragments per tile, a bias-carrying LayerNorm, two images
    "lin4_ln_ff1_1024_gelu": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=48, k=1, norm=LN, WM=1, WN=1, silu=False, out_gelu=True, seed=81),
    "lin4_ln_ff2_2048_resid_wn2": dict(B=2, H=4, W=4, C1=2048, C2=0, Cout=64, k=1, norm=LN, WM=1, WN=2, silu=False, resid=True, seed=82),
    "lin4_ln_bias_1024_b2": dict(B=2, H=4, W=4, C1=1024, C2=0, Cout=32, k=1, norm=LN, WM=1, WN=1, silu=False, ln_bias=True, accum=True, seed=83),
    "lin4_shape_on_the_general_kernel": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=48, k=1, norm=LN, WM=1, WN=1, silu=False, out_gelu=True, seed=81, general=True),
    "layernorm_linear": dict(B=2, H=4, W=4, C1=128, C2=0, Cout=64, k=1, norm=LN, WM=1, WN=1, silu=False, seed=6, out_gelu=True),
    "layernorm_lazy_splitk_linear": dict(B=2, H=4, W=4, C1=128, C2=0, Cout=64, k=1, norm=LN, WM=1, WN=1, silu=False, lazy=1, seed=7),
    "gelu_layernorm_bias_linear": dict(B=2, H=4, W=4, C1=128, C2=0, Cout=64, k=1, norm=LN, WM=1, WN=2, silu=False, pre_gelu=True,
                                       ln_bias=True, seed=6),
}
# the UNet's own layer shapes (B = 1): GPU only
CONV_CASES_FULL = {
    "unet_4x4_1024_s4": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=10),
    "unet_4x4_2048_s4_gate": dict(B=1, H=4, W=4, C1=1024, C2=1024, Cout=1024, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=2, seed=11),
    "unet_8x8_1536": dict(B=1, H=8, W=8, C1=1024, C2=512, Cout=1024, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=12),
    "unet_16x16_768": dict(B=1, H=16, W=16, C1=512, C2=256, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=2, resid=True, seed=13),
    "unet_32x32_512": dict(B=1, H=32, W=32, C1=256, C2=256, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=14),
    "unet_32x32_res_conv": dict(B=1, H=32, W=32, C1=256, C2=256, Cout=256, k=1, norm=NONE, WM=2, WN=2, silu=False, seed=15),
    "unet_ln_ff2_2048": dict(B=1, H=4, W=4, C1=2048, C2=0, Cout=1024, k=1, norm=LN, WM=1, WN=1, silu=False, pre_gelu=True, resid=True, seed=17),
    # the LayerNorm linears as the r04 plan runs them (plain sources): ff1 (+ GELU epilogue), ff2, the merged q | k | v projection
    "unet_ln_ff1_1024": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=2048, k=1, norm=LN, WM=1, WN=1, silu=False, out_gelu=True, seed=65),
    "unet_ln_ff2_2048_plain": dict(B=1, H=4, W=4, C1=2048, C2=0, Cout=1024, k=1, norm=LN, WM=1, WN=1, silu=False, resid=True, seed=66),
    "unet_ln_qkv_1024": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=640, k=1, norm=LN, WM=1, WN=1, silu=False, seed=67),
    "unet_ln_qkv_lazy": dict(B=1, H=4, W=4, C1=1024, C2=0, Cout=640, k=1, norm=LN, WM=1, WN=1, silu=False, lazy=1, seed=18),
    "unet_pair_8x8_1536": dict(B=1, H=8, W=8, C1=1024, C2=512, Cout=1024, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=24, pair=True),
    "unet_pair_4x4_2048_lazy": dict(B=1, H=4, W=4, C1=1024, C2=1024, Cout=1024, k=3, norm=GN_SELF, WM=1, WN=1, S=4, lazy=1, seed=25, pair=True),
    "unet_pair_32x32_512": dict(B=1, H=32, W=32, C1=256, C2=256, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=26, pair=True),
    "unet_pipe_8x8_1536": dict(B=1, H=8, W=8, C1=1024, C2=512, Cout=1024, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=34, pipe=True),
    "unet_pipe_16x16_768": dict(B=1, H=16, W=16, C1=512, C2=256, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=2, resid=True, seed=35, pipe=True),
    "unet_pipe_32x32_512": dict(B=1, H=32, W=32, C1=256, C2=256, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=36, pipe=True),
    "unet_pipe_32x32_256": dict(B=1, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=37, pipe=True, logits=True),
    "unet_pipe_pair_16x16_768": dict(B=1, H=16, W=16, C1=512, C2=256, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=39, pipe=True, pair=True),
    # B = 4 geometry (r03): 32-pixel tiles at 8x8 / 16x16, 64-pixel tiles at 32x32; the 1536-channel frame only fits the chunked
    # (pipelined) kernel
    "unet_b4_pipe_pair_8x8_1536": dict(B=4, H=8, W=8, C1=1024, C2=512, Cout=1024, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=50, pipe=True, pair=True),
    "unet_b4_pipe_16x16_768": dict(B=4, H=16, W=16, C1=512, C2=256, Cout=512, k=3, norm=GN_SLOTS, WM=2, WN=2, resid=True, seed=51, pipe=True),
    "unet_b4_pipe_32x32_512": dict(B=4, H=32, W=32, C1=256, C2=256, Cout=256, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=52, pipe=True, logits=True),
    "unet_b4_pipe_pair_32x32_512": dict(B=4, H=32, W=32, C1=256, C2=256, Cout=256, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=53, pipe=True, pair=True),
    "unet_pipe_pool_32x32_256": dict(B=1, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=58, pipe=True, pool=True),
    "unet_pipe_pool_8x8_1024": dict(B=1, H=8, W=8, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=59, pipe=True, pool=True),
    "unet_b4_pipe_pool_16x16_512": dict(B=4, H=16, W=16, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=60, pipe=True, pool=True),
    "unet_b4_4x4": dict(B=4, H=4, W=4, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SELF, WM=1, WN=1, S=1, seed=16),
    # r06: k_conv3s (csrc/fused_conv3s.h), the recurring single-source geometries with compile-time shapes: full-width strips (tw = W) and
    # 2-D tiles (tw < W), with / without residual, scale-shift, epilogue pooling; `keep_pipe` = the same op on the general pipelined kernel
    "conv3s_32x32_256_strip": dict(B=1, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=90, pipe=True, tw=32),
    "conv3s_32x32_256_tile4x8_resid": dict(B=1, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=91, pipe=True, tw=8, resid=True),
    "conv3s_32x32_256_tile4x8_pool": dict(B=1, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=92, pipe=True, tw=8, pool=True),
    "conv3s_32x32_256_strip_pool_no_ss": dict(B=1, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=93, pipe=True, tw=32, pool=True, ss=False),
    "conv3s_16x16_256_strip": dict(B=2, H=16, W=16, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=94, pipe=True, tw=16, resid=True),
    "conv3s_16x16_256_tile4x4_pool": dict(B=1, H=16, W=16, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=95, pipe=True, tw=4, pool=True),
    "conv3s_16x16_512_tile4x4": dict(B=1, H=16, W=16, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=96, pipe=True, tw=4, resid=True),
    "conv3s_16x16_512_strip_pool": dict(B=1, H=16, W=16, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=97, pipe=True, tw=16, pool=True),
    "conv3s_8x8_1024_resid": dict(B=1, H=8, W=8, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=104, pipe=True, tw=8, resid=True),
    "conv3s_8x8_512_pool": dict(B=1, H=8, W=8, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=105, pipe=True, tw=8, pool=True),
    "conv3s_16x16_512_tile4x4_pool": dict(B=1, H=16, W=16, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=103, pipe=True, tw=4, pool=True),
    "conv3s_8x8_512": dict(B=2, H=8, W=8, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=98, pipe=True, tw=8, resid=True),
    "conv3s_8x8_1024_pool": dict(B=1, H=8, W=8, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=99, pipe=True, tw=8, pool=True),
    "conv3s_b2_32x32_256_tile8x8_wn2": dict(B=2, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=100, pipe=True, tw=8, pool=True),
    "conv3s_16x16_256_strip_pool": dict(B=1, H=16, W=16, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=106, pipe=True, tw=16, pool=True),
    "conv3s_16x16_256_tile4x4": dict(B=2, H=16, W=16, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=107, pipe=True, tw=4, resid=True, ss=False),
    "conv3s_16x16_512_strip": dict(B=1, H=16, W=16, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=108, pipe=True, tw=16),
    "conv3s_b2_32x32_256_strip2_wn2": dict(B=2, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=109, pipe=True, tw=32, resid=True),
    "conv3s_b2_32x32_256_strip2_wn2_pool": dict(B=2, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=110, pipe=True, tw=32, pool=True),
    "conv3s_b3_32x32_256_tile8x8_wn2": dict(B=3, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=4, WN=2, seed=111, pipe=True, tw=8),
    # B >= 2 tiles at 16x16 (8 rows x 4 columns) and 8x8 (4 rows)
    "conv3s_b2_16x16_256_tile8x4": dict(B=2, H=16, W=16, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=1, seed=130, pipe=True, tw=4, resid=True),
    "conv3s_b2_16x16_256_tile8x4_pool": dict(B=2, H=16, W=16, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=1, seed=131, pipe=True, tw=4, pool=True),
    "conv3s_b4_16x16_256_tile8x4_wn2": dict(B=4, H=16, W=16, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=132, pipe=True, tw=4),
    "conv3s_b4_16x16_256_tile8x4_wn2_pool": dict(B=4, H=16, W=16, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=133, pipe=True, tw=4, pool=True, ss=False),
    "conv3s_b2_16x16_512_tile8x4": dict(B=2, H=16, W=16, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=134, pipe=True, tw=4, resid=True),
    "conv3s_b2_16x16_512_tile8x4_pool": dict(B=2, H=16, W=16, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=135, pipe=True, tw=4, pool=True),
    "conv3s_b2_8x8_512_rows4": dict(B=2, H=8, W=8, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=2, WN=1, seed=136, pipe=True, tw=8),
    "conv3s_b2_8x8_512_rows4_pool": dict(B=2, H=8, W=8, C1=512, C2=0, Cout=512, k=3, norm=GN_SLOTS, WM=2, WN=1, seed=137, pipe=True, tw=8, pool=True),
    "conv3s_b2_8x8_1024_rows4": dict(B=2, H=8, W=8, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SLOTS, WM=2, WN=1, seed=138, pipe=True, tw=8, resid=True),
    "conv3s_b2_8x8_1024_rows4_pool": dict(B=2, H=8, W=8, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SLOTS, WM=2, WN=1, seed=139, pipe=True, tw=8, pool=True),
    "conv3s_b4_8x8_1024_rows4_wn2": dict(B=4, H=8, W=8, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=140, pipe=True, tw=8),
    "conv3s_b4_8x8_1024_rows4_wn2_pool": dict(B=4, H=8, W=8, C1=1024, C2=0, Cout=1024, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=141, pipe=True, tw=8, pool=True),
    # r06: k_conv3s_rc -- conv1 on the concat of two sources + the block's res_conv in the same workgroups (the pipelined pairs of the B = 1 plan)
    "conv3s_rc_32x32_512_tile4x8": dict(B=2, H=32, W=32, C1=256, C2=256, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=121, pipe=True, pair=True, tw=8, ss=False),
    "conv3s_rc_16x16_768_tile4x4": dict(B=1, H=16, W=16, C1=512, C2=256, Cout=512, k=3, norm=GN_SLOTS, WM=1, WN=2, seed=123, pipe=True, pair=True, tw=4),
    "conv3s_rc_8x8_1536": dict(B=1, H=8, W=8, C1=1024, C2=512, Cout=1024, k=3, norm=GN_SLOTS, WM=1, WN=1, seed=124, pipe=True, pair=True, tw=8, ss=False),
    "conv3s_geometry_on_the_general_kernel": dict(B=1, H=32, W=32, C1=256, C2=0, Cout=256, k=3, norm=GN_SLOTS, WM=2, WN=2, seed=90, pipe=True, tw=32, keep_pipe=True),
}

"""References and per-element bounds for the normalisation / softmax / pack kernels of sparsefusion_amd/csrc/unet_ops.hip and attn_ln.h
(OP_GN_ACT, OP_GN_FINALIZE, OP_LN, OP_ATTN, ELTWISE modes 5 and 6), in the pattern of tests/fused_cases.py: a float64 reference that
rounds where the kernel rounds, and for EVERY output element a bound derived from the roundings on the kernel's path.  No constant here
is fitted to a kernel's output; the measured margins are in profiles/norm_parity_margins.log.

Derivation.  u = 2^-24 (fp32 round to nearest); an instruction the ISA documents as accurate to 1 ulp (v_exp_f32, v_rcp_f32, v_rsq_f32) is
2 u -- the figures of fused_cases.py, every term first order in u.

(a) GroupNorm (k_gn_apply, k_gn_one):  y = ((v - mean) * rstd * gamma + beta) * (scale + 1) + shift,  s = SiLU(y).
  v - mean cancels, so a rounding acts on the magnitude of the TERMS, not of y:
      M = ((|v| + |mean|) * rstd * |gamma| + |beta|) * |scale + 1| + |shift|.
  Roundings: mean double -> float, v - mean, * rstd, * gamma, + beta, scale + 1, * (scale + 1), + shift: N_AFF = 8 (a contracted fma has fewer).
  rstd = rsqrtf((float) var + eps): var's conversion, the add (u each on the argument = u on rstd) and v_rsq (2 u): 3 u.
  A channel of the second source is v = src2 * src2_scale: one rounding, dx = u |v| (a plain first source: dx = 0).
  Statistics: a thread adds n_t float4 chunks in fp32 -- s += (v0 + v1) + (v2 + v3) is a chain of n_t + 2 additions, q = fma(v, v, q) one of
  4 n_t -- then (k_gn_stats, k_gn_one) six fp32 shuffle levels; everything above is double.  A chain of n additions is off by at most
  n u sum|terms|:
      |d sum| <= (n_t + 8) u sum|v| + sum dx,      |d sumsq| <= (4 n_t + 6) u sum v^2 + 2 sum |v| dx
      d mean = d sum / n,    d var = d sumsq / n + 2 |mean| d mean,    d rstd / rstd = d var / (2 (var + eps))
  and they move y by  |dy/dmean| d mean = rstd |gamma (scale + 1)| d mean  and  |dy/drstd| d rstd = |v - mean| |gamma (scale + 1)| d rstd:
      d(y) = u (N_AFF + 3) M + rstd |gamma (scale + 1)| (dx + d mean) + |v - mean| rstd |gamma (scale + 1)| (d rstd / rstd).
  n_t by kernel (gn_geometry below restates run_gn): NCH for k_gn_one, ceil(per / 256) for k_gn_stats, ceil(HW / (slabs * ppi)) for
  k_gn_stats_px.  Statistics from a conv epilogue (flag 2): a (128-pixel tile, group) partial is an fp32 chain of at most 32 values per thread
  (k_conv_glds / k_conv3_halo: 128 / RPP rows x 4 columns, RPP >= 16; k_conv_lds: 16 rows + 2 + 4 shuffle levels), doubles above:
  READY_COUNTS.
  SiLU, v / (1 + __expf(-v)): the product v * log2 e is off by u, which moves the exponential by |v| u; + 2 u (v_exp) + u (the add) + the
  division (correctly rounded: u; v_rcp and a product: 3 u): (|y| + 6) u |s| on top of what d(y) does through the local slope silu'(y), with
  |silu''| <= 1/2 for the remainder -- fused_cases.py (a):
      d(s) = |silu'(y)| d(y) + d(y)^2 / 4 + (|y| + 6) u |s|.
(b) LayerNorm (k_layernorm, k_layernorm_wave, k_layernorm_w256; two-pass variance, all fp32): the chains of fused_cases.py, N_SUM_LN = 24 and
  N_SQ_LN = 72 (they cover 8 values per thread + 6 + 3 levels + the division); the squares are of (v - mean), all positive:
  d rstd / rstd = N_SQ_LN u / 2; roundings of (v - mean) * rstd * gain + bias: 4, + 3 u for rstd; a GELU in front: dx = 8 u |v| (fused_cases (c)).
(c) softmax rows (k_softmax_rows):  t = x * scale (u |t|),  a = t - max (u |a|; the maximum itself is off by u |max|): d a <= u (|t| + |max| + |a|);
  expf (<= 1 ulp): e is off by (d a + 2 u) e; the sum: ceil(N / 256) + 6 + 3 additions of positive terms, each of which is itself off by at most
  max_j (d a_j + 2 u); 1 / sum: 2 u; the product: u:
      d p / p = d a + max_j d a_j + (ceil(N / 256) + 16) u,
  plus one fp32 minimum normal (2^-126) absolute for a flushed subnormal.
(d) the 16-token attention core (k_attn16): q * scale (u), 64 chained fma per score: d sim = 65 u sum_d |q k| scale; softmax as (c) with a serial
  sum of J <= 24 terms; the output is a chain of J fma of p_j v_j:
      d out = sum_j |p_j v_j| (d p_j / p_j + J u),    d p / p = d sim + 3 max_j d sim_j + u (|a| + max|a|) + (J + 9) u
  (a score and the maximum it is taken from: d sim + max d sim; the same again, at most, for every term of the denominator).
A bf16 output is checked as |got - want| <= half_ulp_bf16(want) + delta for every element (check_bf16), and the share of elements with
got != bf16(want) -- those the bound accepted included -- is capped at MISMATCH_MAX per case."""
import math

import torch

U24 = 2.0 ** -24
N_AFF_GN = 8
N_SUM_LN, N_SQ_LN = 24, 72                 # fused_cases.py
READY_COUNTS = (32, 32)                    # (a): partial sums of a conv epilogue
MISMATCH_MAX = 1e-3
OP_CONV, OP_GN_ACT, OP_LN, OP_ATTN, OP_ELTWISE, OP_GN_FINALIZE = 1, 2, 3, 5, 7, 18


# ---------------------------------------------------------------------------------------------------------------------------------
# run_gn's geometry rule (sparsefusion_amd/csrc/unet_ops.hip), restated: which kernel takes an OP_GN_ACT and how many float4 chunks a
# thread of its statistics pass adds up in fp32.  tests/test_plans_cpu.py checks it on the shapes the GPU cases are written for.
def gn_geometry(B, HW, C1, C2=0, G=8, flags=0, lazy=0):
    C = C1 + C2
    assert C % (4 * G) == 0 and C1 % 4 == 0
    chunks, c4 = HW * (C // G) // 4, C // 4
    if not (flags & (2 | 4)) and (B * G >= 256 or (B * G >= 64 and B * HW * C <= (1 << 19)) or (flags & 8)) and chunks <= 1024 * 16:
        for nt, nch in ((256, 2), (256, 4), (256, 8), (256, 16), (1024, 8), (1024, 16)):
            if chunks <= nt * nch:
                return dict(kernel="k_gn_one", NT=nt, NCH=nch, n_t=nch, chunks=chunks)
    if flags & 2:
        assert not C2 and not lazy
        return dict(kernel="ready", n_t=None, chunks=chunks)
    if not C2 and not lazy and C // G <= 16 and c4 <= 256 and 256 % c4 == 0:
        ppi = 256 // c4
        slabs = min(max(HW // (ppi * 16), 1), 1024)
        per = (HW + slabs - 1) // slabs
        return dict(kernel="k_gn_stats_px", slabs=slabs, ppi=ppi, n_t=(per + ppi - 1) // ppi, chunks=chunks)
    per_block = 256 if lazy == 1 else 2048
    slices = (chunks + per_block - 1) // per_block
    want, max_slices = 128 // (B * G), (chunks + 255) // 256
    if slices < want:
        slices = min(want, max_slices)
    slices = max(slices, 1)
    per = (chunks + slices - 1) // slices
    return dict(kernel="k_gn_stats", slices=slices, n_t=(per + 255) // 256, chunks=chunks)


def stat_counts(geo):
    """(additions on the sum, on the sum of squares) of the fp32 part of a statistics pass, derivation (a)."""
    return READY_COUNTS if geo["kernel"] == "ready" else (geo["n_t"] + 8, 4 * geo["n_t"] + 6)


# ---------------------------------------------------------------------------------------------------------------------------------
def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def half_ulp_bf16(w):
    """Half the spacing of bf16 (8 significant bits) at |w|, float64; subnormal spacing below 2^-126."""
    e = torch.frexp(w.abs())[1].double() - 1            # floor(log2 |w|); frexp(0) = (0, 0)
    e = torch.where(w == 0, torch.full_like(e, -126.0), e).clamp(min=-126.0)
    return torch.exp2(e - 8)


def silu64(y, dy):
    sg = torch.sigmoid(y)
    s = y * sg
    return s, (sg * (1 + y * (1 - sg))).abs() * dy + dy * dy / 4 + (y.abs() + 6) * U24 * s.abs()


def gn_act_ref64(x1, x2, s2_scale, G, gamma, beta, eps, counts, ss=None, silu=True, dx1=None, stats=None):
    """x1 [B, HW, C1] (float64: the exact value of the first source; dx1 its uncertainty when it is evaluated lazily), x2 [B, HW, C2] fp32 or
    None, ss = (scale [B, C], shift [B, C]) or None, counts = stat_counts(...).  Returns want, delta [B, HW, C], the float64 (sum, sum of
    squares) per (image, group) [B, G, 2] and their bound.  stats [B, G, 2] float64 = the ready-made statistics an op with flag 2 READ
    (tests/vae_plan_cases.py): want is then evaluated on them, exactly as k_gn_apply does, and they add nothing to delta; the sums returned
    are still those of the tensor, under `counts`."""
    B, HW, C1 = x1.shape
    C = C1 + (x2.shape[2] if x2 is not None else 0)
    Cg, n = C // G, HW * (C // G)
    sc2, eps32 = f32(s2_scale), f32(eps)
    n_sum, n_sq = counts
    g64, b64 = gamma.double(), beta.double()
    want, delta = torch.empty(B, HW, C, dtype=torch.float64), torch.empty(B, HW, C, dtype=torch.float64)
    sums, sums_bound = torch.empty(B, G, 2, dtype=torch.float64), torch.empty(B, G, 2, dtype=torch.float64)
    grp = lambda t: t.view(HW, G, Cg)
    for b in range(B):                                   # per image: the big cases would not fit otherwise
        x, dx = x1[b].double(), (dx1[b] if dx1 is not None else torch.zeros(HW, C1, dtype=torch.float64))
        if x2 is not None:
            v2 = x2[b].double() * sc2
            x, dx = torch.cat([x, v2], 1), torch.cat([dx, U24 * v2.abs()], 1)
        s1, s2, sa = grp(x).sum((0, 2)), grp(x * x).sum((0, 2)), grp(x.abs()).sum((0, 2))
        d_s1 = n_sum * U24 * sa + grp(dx).sum((0, 2))
        d_s2 = n_sq * U24 * s2 + 2 * grp(x.abs() * dx).sum((0, 2))
        sums[b], sums_bound[b] = torch.stack([s1, s2], -1), torch.stack([d_s1, d_s2], -1)
        if stats is not None:
            s1, s2, d_s1, d_s2 = stats[b, :, 0].double(), stats[b, :, 1].double(), torch.zeros_like(d_s1), torch.zeros_like(d_s2)
        mean, ex2 = s1 / n, s2 / n
        var = (ex2 - mean * mean).clamp(min=0)
        mean32, var32 = mean.float().double(), var.float().double()       # the kernel's rounding points
        rstd = (var32 + eps32).rsqrt()
        d_mean = d_s1 / n
        d_rel = (d_s2 / n + 2 * mean.abs() * d_mean) / (2 * (var32 + eps32))
        ex = lambda t: t.view(1, G, 1).expand(HW, G, Cg).reshape(HW, C)
        mean32, rstd, d_mean, d_rel = ex(mean32), ex(rstd), ex(d_mean), ex(d_rel)
        if ss is not None:
            sc, sh = ss[0][b].double() + 1, ss[1][b].double()
        else:
            sc, sh = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        a = x - mean32
        y = (a * rstd * g64 + b64) * sc + sh
        mag = ((x.abs() + mean32.abs()) * rstd * g64.abs() + b64.abs()) * sc.abs() + sh.abs()
        slope = rstd * (g64 * sc).abs()
        dy = U24 * (N_AFF_GN + 3) * mag + slope * (dx + d_mean) + a.abs() * slope * d_rel
        want[b], delta[b] = silu64(y, dy) if silu else (y, dy)
    return want, delta, sums, sums_bound


def gn_chain_f32(x, G, gamma, beta, eps, ss=None, silu=True, n_t=8):
    """An fp32 restatement of the kernel chain on the CPU (k_gn_stats order: per-thread fp32 sums of n_t float4 chunks, doubles above; then
    k_gn_apply's expression in fp32, unfused) -> bf16.  x [B, HW, C] fp32.  Used to show that the REFERENCE ALONE leaves the mismatch share
    under MISMATCH_MAX (tests/test_plans_cpu.py); it is not a kernel."""
    B, HW, C = x.shape
    Cg = C // G
    xg = x.view(B, HW, G, Cg).permute(0, 2, 1, 3).reshape(B * G, -1, 4)                 # float4 chunks of a group, pixel-major
    nchunk = xg.shape[1]
    per = 256 * n_t
    pad = (-nchunk) % per
    xp = torch.cat([xg, torch.zeros(B * G, pad, 4)], 1).view(B * G, -1, n_t, 256, 4)     # [bg][block][k][thread][4]
    s = torch.zeros(xp.shape[0], xp.shape[1], 256)
    q = torch.zeros_like(s)
    for k in range(n_t):
        v = xp[:, :, k]
        s = s + ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3]))
        for j in range(4):
            q = q + v[..., j] * v[..., j]           # (an fma in the kernel: one rounding less)
    n = HW * Cg
    m = s.double().sum((1, 2)) / n
    var = q.double().sum((1, 2)) / n - m * m
    mean = m.float().view(B, 1, G, 1)
    rstd = ((var.clamp(min=0).float() + torch.tensor(eps, dtype=torch.float32)).rsqrt()).view(B, 1, G, 1)
    y = ((x.view(B, HW, G, Cg) - mean) * rstd).view(B, HW, C) * gamma + beta
    if ss is not None:
        y = y * (ss[0] + 1.0)[:, None] + ss[1][:, None]
    if silu:
        y = y / (1.0 + torch.exp(-y))
    return y.to(torch.bfloat16)


def layernorm_ref64(x, gain, bias, eps, pre_gelu=False):
    """x [R, C] fp32 -> want, delta (before an fp32 residual add), derivation (b)."""
    x64 = x.double()
    dx = torch.zeros_like(x64)
    if pre_gelu:
        dx = 8 * U24 * x64.abs()
        x64 = 0.5 * x64 * (1.0 + torch.erf(x64 * 0.7071067811865476))
    mean = x64.mean(1, keepdim=True)
    var = (x64 - mean).pow(2).mean(1, keepdim=True)
    rstd = (var + f32(eps)).rsqrt()
    r2 = (x64 * x64).mean(1, keepdim=True) / var
    g64 = gain.double()
    b64 = bias.double() if bias is not None else torch.zeros_like(g64)
    y = (x64 - mean) * rstd * g64 + b64
    mag = (x64.abs() + mean.abs()) * rstd * g64.abs() + b64.abs()
    dy = U24 * ((4 + 3 + N_SQ_LN / 2) * mag + N_SUM_LN * r2.sqrt() * g64.abs()) + rstd * g64.abs() * (dx + dx.mean(1, keepdim=True))
    return y, dy


def softmax_ref64(x, scale, serial=None):
    """x [R, N] fp32, scale a float -> want, delta of softmax(scale * x) per row, derivation (c)."""
    N = x.shape[1]
    t = x.double() * f32(scale)
    mx = t.max(1, keepdim=True).values
    a = t - mx
    p = torch.softmax(t, 1)
    da = U24 * (t.abs() + mx.abs() + a.abs())
    rel = da + da.max(1, keepdim=True).values + (math.ceil(N / 256) + 16) * U24
    return p, p * rel + 2.0 ** -126


def attn16_ref64(q, k, v, scale):
    """q [B, H, 16, D] fp32, k / v [B, H, J, D] fp32 -> want, delta [B, H, 16, D], derivation (d)."""
    J = k.shape[2]
    sc = f32(scale)
    q64, k64, v64 = q.double() * sc, k.double(), v.double()
    sim = torch.einsum("bhid,bhjd->bhij", q64, k64)
    dsim = 65 * U24 * torch.einsum("bhid,bhjd->bhij", q64.abs(), k64.abs())
    a = sim - sim.max(-1, keepdim=True).values
    p = torch.softmax(sim, -1)
    rel = dsim + 3 * dsim.max(-1, keepdim=True).values + U24 * (a.abs() + a.abs().max(-1, keepdim=True).values) + (J + 9) * U24
    want = torch.einsum("bhij,bhjd->bhid", p, v64)
    delta = torch.einsum("bhij,bhjd->bhid", p * (rel + J * U24), v64.abs())
    return want, delta


# ---------------------------------------------------------------------------------------------------------------------------------
def check_bf16(name, got, want, delta, old=None, cap=MISMATCH_MAX, log=True):
    """got: bf16 (or its float view); want, delta float64.  Asserts finiteness, |got - want| <= half_ulp_bf16(want) + delta for every element
    and the mismatch cap; prints the margin line of profiles/norm_parity_margins.log.  old = (rtol, atol): the figures of the earlier
    whole-tensor allclose on the same data, printed beside the new ones.  Returns the figures."""
    g = got.double().reshape(want.shape)
    assert bool(torch.isfinite(g).all()), f"{name}: output not finite"
    hu = half_ulp_bf16(want)
    bound = hu + delta
    err = (g - want).abs()
    ratio = err / bound
    worst = int(ratio.argmax())
    mism = float((g != want.float().to(torch.bfloat16).double()).double().mean())
    med = float((delta / hu).median())
    used = float(((err - hu) / delta).max())              # the share of delta the worst element needs beyond its half ulp (<= 1 asserted through the bound)
    line = f"margin {name}: worst err/bound {float(ratio.reshape(-1)[worst]):.3f} worst (err - half_ulp)/delta {used:.3f} mismatch {mism:.2e} median delta/half_ulp {med:.2e}"
    if old is not None:
        rtol, atol = old
        line += f" | old allclose: worst err/(atol + rtol |want|) {float((err / (atol + rtol * want.abs())).max()):.3f} mean err {float(err.mean()):.2e}"
    if log:
        print(line)
    bad = int((err > bound).sum())
    assert bad == 0, (f"{name}: {bad} of {err.numel()} elements outside half_ulp + delta; worst err / bound {float(ratio.reshape(-1)[worst]):.3g} "
                      f"(got {float(g.reshape(-1)[worst]):.6g} want {float(want.reshape(-1)[worst]):.6g}) at flat index {worst} of shape {tuple(want.shape)}")
    assert mism <= cap, f"{name}: share of elements with got != bf16(want) {mism:.3g} > {cap}"
    return dict(worst=float(ratio.reshape(-1)[worst]), used=used, mismatch=mism, median=med)


def check_stats(name, got, sums, sums_bound):
    """The statistics buffer p[7] after k_gn_stats / k_gn_stats_px / k_gn_finalize: float64 sums to the derived bound."""
    err = (got.double().view(sums.shape) - sums).abs()
    ratio = float((err / sums_bound.clamp(min=1e-300)).max())
    print(f"margin {name}: statistics worst err/bound {ratio:.3f}")
    assert bool((err <= sums_bound).all()), f"{name}: statistics outside their bound, worst err / bound {ratio:.3g}"


# ---------------------------------------------------------------------------------------------------------------------------------
_KEEP = []          # device tensors referenced by raw pointer must outlive the launch


def mkop(type_, flags=0, p=(), i=(), f=()):
    from sparsefusion_amd import _lib
    o = _lib.SfOp()
    o.type, o.flags = type_, flags
    for k, v in enumerate(p):
        if torch.is_tensor(v):
            _KEEP.append(v)
        o.p[k] = v.data_ptr() if torch.is_tensor(v) else (v or None)
    for k, v in enumerate(i):
        o.i[k] = int(v)
    for k, v in enumerate(f):
        o.f[k] = float(v)
    return o


def run(ops):
    """sf_plan_run; returns the status code instead of raising when it is not SF_OK (a refused op)."""
    from sparsefusion_amd import _lib
    arr = (_lib.SfOp * len(ops))(*ops)
    rc = _lib.lib().sf_plan_run(arr, len(ops), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def pack_conv(w, dev):
    """sf_conv_pack_weights (host): [Cout, Cin, kh, kw] fp32 -> (packed int16 tensor on dev, Cin padded to 32)."""
    from sparsefusion_amd import _lib
    lib = _lib.lib()
    co, ci, kh, kw = w.shape
    cpad = (ci + 31) // 32 * 32
    buf = torch.empty(lib.sf_conv_packed_elems(co, cpad, kh, kw), dtype=torch.int16)
    _lib.check(lib.sf_conv_pack_weights(w.contiguous().data_ptr(), co, ci, cpad, kh, kw, buf.data_ptr()))
    return buf.to(dev), cpad

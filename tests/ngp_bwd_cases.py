"""References and per-element bounds for the fused Instant-NGP render backward (sf_ngp_render_backward of sparsefusion_amd/csrc/ngp_render.hip:
k_ngp_composite_bwd_wave of ngp_composite_wave.h, then k_ngp_field_bwd_mfma of ngp_bwd_mfma.h), in the pattern of tests/norm_cases.py: a float64
reference that rounds where the kernel rounds, and for EVERY output element a bound derived from the roundings on the kernel's path.  No
constant here is fitted to a kernel's output; the measured margins are in profiles/ngp_bwd_parity_margins.log.

Derivation.  u = 2^-24 (fp32 round to nearest), every term first order in u unless said otherwise.  A chain of n fp32 additions / fmas is off by
at most n u sum|terms|.  expf of the device library and of the host libm is within 1 ulp.  Every fp32 result may be subnormal (rounded to 2^-149, or flushed): 2^-126
absolute per fp32 rounding on top of the relative terms below.

(A) Composite backward (one wave per ray, sorted positions m = 0 .. 2T - 1).  Rounded to fp32 in the reference exactly as in the kernel: the
  deltas d_m = z_{m+1} - z_m (the last one (far - near) / T), x = -d s, e = expf(x), a = 1 - e, one = (1 - a) + 1e-15f, tr = (float) excl,
  w = a tr.  Float64: the exclusive product scan excl_m = prod_{j<m} one_j (the kernel multiplies doubles too: 2^-53 per level, ignored),
  av = gI . c - bg (gI0 + gI1 + gI2) + gW, t = av w, after_m = sum_{j>m} t_j, da = av tr - after / one, dsig = da d e, drgb = w gI.
  Uncertainties (kernel value against reference value):
    e:    the kernel's expf is within 1 ulp of the exact value, the reference's rounding within half: d_e = 1.5 ulp(e) + 2^-126.
    a:    1 - e is exact for e >= 1/2 (Sterbenz): d_a = d_e; for e < 1/2 a lies in (1/2, 1], where the grid is 2^-24: d_a = d_e + u.
    one:  1 - a is exact (a is a multiple of 2^-24 in [0, 1]), and it is either 0 or >= 2^-24, where adding 1e-15f changes nothing:
          d_one = d_a.  For e < 2^-26 both sides have a = 1 and one = 1e-15f exactly: d_a = d_one = 0 (the saturated regime).
    tr:   the kernel's scan multiplies ones within [lo_j, hi_j] = [max(one_j - d_one_j, 1e-15f), one_j + d_one_j]:
          d_tr_m = max(prod hi_j - excl_m, excl_m - prod lo_j) + u tr_m + 2^-126  (NOT first order: an `one` of a few 2^-24 is uncertain by its
          own size).
    w:    d_w = a d_tr + tr d_a + u |w|.
    av:   three products, the product bg gsum, gsum's two additions and four additions / subtractions, on the magnitude of the TERMS:
          d_av = 10 u A,  A = sum_i |gI_i c_i| + |bg| sum_i |gI_i| + |gW|.
    t, after (doubles):  d_t = |av| d_w + |w| d_av,  d_after_m = sum_{j>m} d_t_j.
    q = after / one:  |after_k / one_k - after / one| <= d_after / lo + |after| d_one / (one lo)  -- the conditioning: for one ~ 2^-24 k the
          quotient is uncertain by |after / one| 2^-24 / one.
    da = av tr - (float) q:  each rounding acts on the magnitudes of the two terms, not on their difference:
          d_da = tr d_av + |av| d_tr + d_q + u |q| + 2 u (|av tr| + |q|).
    dsig = da d e (d is the same fp32 number on both sides):  d_dsig = |d e| d_da + |da d| d_e + 2 u |dsig|.
    drgb = w gI:  d_drgb = |gI| d_w + u |drgb|.
  A miss ray (near >= far) goes through the same arithmetic in the kernel and in the reference; `mask` excludes it from the checks.

(B) Field backward, per point.  Exact inputs: the fp32 features F [32] of the sorted sample, the fp32 weights, the fp32 dsig / drgb of stage A
  as the GPU left them.  z1 = W0 F + b0, h1 = relu(z1), z2 = W1 h1 + b1, h2 = relu(z2), out = W2 h2 + b2 (float64).
  ReLU margins (bias + K fmas on the matrix cores or the VALU, K + 2 covers any summation order):
      m1 = 34 u (|W0| |F| + |b0|),                      d_h1 = m1 where the unit is active or ambiguous, 0 where it is off,
      m2 = 66 u (|W1| h1 + |b1|) + |W1| d_h1,           d_h2 likewise,            d_out = 66 u (|W2| h2 + |b2|) + |W2| d_h2.
  A unit with |z| <= m is AMBIGUOUS: the kernel may have taken either side.  Toggling it moves h by at most m (inside d_h), so the forward
  values are shared by all candidate masks; the backward is evaluated for each of the 2^k candidates of a point with k ambiguous units.
  d(out):  pre = out0 + blob(x),  blob = 5 expf(-|x|^2 / 0.08f)  (|x|^2: 5 roundings on positive terms, the division, expf at 2 u, the
      product: d_blob = blob ((6 |x|^2 / 0.08 + 4) u)),  d_pre = d_out0 + d_blob + u |pre|;
      dout0 = dsig expf(clamp(pre, -15, 15)):  d = |dout0| (d_pre + 3 u)  (expf 2 u, one product);
      sg = 1 / (1 + expf(-o)) (expf 2 u, the addition, the division: 4 u), d_sg = 4 u sg + sg (1 - sg) d_out;  s1 = 1 - sg: d_s1 = d_sg + u s1;
      dout_c = drgb_c sg s1:  d = |drgb_c| (s1 d_sg + sg d_s1 + 2 u sg s1).
  dh2 = (W2^T dout) .* mask2: a chain of 4: d_dh2 = (4 u |W2|^T |dout| + |W2|^T d_dout) .* mask2;   dh1 = (W1^T dh2) .* mask1 and
  d(feat) = W0^T dh1 are chains of 64: d = 64 u |W|^T |.| + |W|^T d_(.).  d(feat) is zero for a point outside the unit box.  (Behind an opaque
  sample dsig is far below 2^-126: every operand and result may be subnormal or flushed, 2^-126 absolute each, carried through |W| like d_(.).)
  The GPU's d(feat) row must lie within the bound of at least one candidate; the closest candidate is taken as the kernel's mask.  Where several
  candidates fit, the largest difference of their dh2 / dh1 to the chosen one is added to d_dh2 / d_dh1 for the weight gradients.  A point with
  k > 4 is left out: its row is not checked, and |W2|^T |dout| (and that through |W1|) is added to d_dh2 (d_dh1).

  Weight and bias gradients, dW2 = sum_p dout h2^T, dW1 = sum_p dh2 h1^T, dW0 = sum_p dh1 F^T, db = sum_p d(.).  bwd_geometry restates the
  launch geometry of sf_ngp_render_backward; a wave that runs n trips accumulates 32 n points per element (fp32 fma / MFMA accumulation: 32 n
  roundings; a bias: 32 additions per trip and one per trip into the running sum; + 2 spare): per wave
      E_w = (33 n + 2) u sum_{p in wave} |t_p| + sum_{p in wave} (first-order terms of the factors: d_dh2 |h1| + |dh2| d_h1, ...).
  Every wave's sum S_w is rounded once to 2^-44 fixed point: 2^-45 per wave and chunk.  A wave whose |S_w| can reach thr_mlp (|S_w| + E_w >= thr)
  takes an fp32 atomic instead: k such waves form a chain of k additions in any order, k u sum |S_w| over them, and the conversion adds the
  fixed-point part to them with two more roundings: the final rounding is u |want| without, 3 u |want| with atomics."""
import math

import torch

U24 = 2.0 ** -24
TINY = 2.0 ** -126
FB_PTS = 32
K1, K2 = 32, 64
MAX_AMBIGUOUS = 4                         # candidates per point: 2^k
AMBIGUOUS_CAP, LEFT_OUT_CAP = 1e-2, 1e-4  # conditions on the reference alone (share of live points)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


EPS15 = f32(1e-15)
C008 = f32(0.08)


# ---------------------------------------------------------------------------------------------------------------------------------
# sf_ngp_render_backward's launch geometry (sparsefusion_amd/csrc/ngp_bwd_plan.h), restated.  tests/test_plans_cpu.py checks it against CASES,
# tests/test_hostemu_ngp_bwd.py against the C++ functions themselves.
def fix_thr(max_addends):
    """sf_fix_thr (sf_fix.h): the largest power of two <= 2^18 / max_addends."""
    t = 262144.0
    while t > 2.0 ** -40 and t * max_addends > 262144.0:
        t *= 0.5
    return t


def bwd_plan(N, want_chunks=2):
    """ngp_bwd_plan: ray index where every chunk starts, and N at the end."""
    ok = lambda rays, k: k >= 1 and rays % k == 0 and (rays // k) % 256 == 0 and rays // k >= 2048
    equal = lambda k: [i * (N // k) for i in range(k + 1)]
    k = (N + 8191) // 8192
    while want_chunks < k <= 64:
        if ok(N, k):
            return equal(k)
        k += 1
    k = want_chunks
    while k > 1 and not ok(N, k):
        k -= 1
    if N // k > 8192:
        per = 8192
        if (N + per - 1) // per > 64:
            per = (((N + 63) // 64 + 255) // 256) * 256
        n = (N + per - 1) // per
        return [i * per for i in range(n)] + [N]
    return equal(k)


def bwd_geometry(N, T, starts=None, grids=None, thr=None):
    """Chunks (first point, points, trips, workgroups) of the field backward, thr_mlp, and per point the wave that accumulates it: wave 4 b + w of
    a chunk takes trips 4 b + w + 4 grid i.  starts / grids / thr override the host's rule (the emulation launches any geometry)."""
    T2 = 2 * T
    starts = bwd_plan(N) if starts is None else starts
    chunks, wave, coef, base = [], [], [], 0
    for c in range(len(starts) - 1):
        p0, P = starts[c] * T2, (starts[c + 1] - starts[c]) * T2
        trips = (P + FB_PTS - 1) // FB_PTS
        grid = grids[c] if grids is not None else ((trips + 3) // 4 if trips < 1024 else 256)
        chunks.append((p0, P, trips, grid))
        trip = torch.arange(P) // FB_PTS
        wl = trip % (4 * grid)
        n_trips_w = (trips - wl + 4 * grid - 1) // (4 * grid)           # trips the wave of this point runs
        wave.append(base + wl)
        coef.append((33.0 * n_trips_w.double() + 2.0) * U24)
        base += 4 * grid
    return dict(N=N, T=T, chunks=chunks, thr=fix_thr(4.0 * 256.0 * len(chunks)) if thr is None else thr, wave=torch.cat(wave), coef=torch.cat(coef),
                n_waves=base)


# the GPU cases of tests/test_gpu_ngp_bwd.py: rays x T and the geometry they are written for (first point, points, trips, workgroups per chunk)
CASES = {
    "ragged": dict(N=37, T=11, chunks=[(0, 814, 26, 7)], thr=256.0, max_trips_per_wave=1),
    "golden": dict(N=256, T=64, chunks=[(0, 32768, 1024, 256)], thr=256.0, max_trips_per_wave=1),
    "two_chunks": dict(N=4096, T=16, chunks=[(0, 65536, 2048, 256), (65536, 65536, 2048, 256)], thr=128.0, max_trips_per_wave=2),
    "unequal_chunks": dict(N=10000, T=8, chunks=[(0, 131072, 4096, 256), (131072, 28928, 904, 226)], thr=128.0, max_trips_per_wave=4),
}


# ---------------------------------------------------------------------------------------------------------------------------------
def _ulp32(v):
    """Spacing of fp32 at |v| (float64 tensor), subnormal spacing below 2^-126."""
    e = torch.frexp(v.abs())[1].double() - 1
    e = torch.where(v == 0, torch.full_like(e, -126.0), e).clamp(min=-126.0)
    return torch.exp2(e - 23)


def _suffix_excl(t):
    """sum_{j > m} t_j along the last axis, summed from the back (no term in front of m + 1 enters: subtracting t_m from an inclusive sum would
    cancel where t_m is many orders above what lies behind an opaque sample)."""
    incl = torch.flip(torch.cumsum(torch.flip(t, [-1]), -1), [-1])
    return torch.cat([incl[..., 1:], torch.zeros_like(t[..., :1])], -1)


def _excl_prod(f):
    return torch.cat([torch.ones_like(f[:, :1]), torch.cumprod(f, 1)[:, :-1]], 1)


def composite_bwd_ref64(z, sig, rgb, nears, fars, T, bg, gi, gw=None):
    """z, sig [N, 2T], rgb [N, 2T, 3], nears, fars [N], gi [N, 3], gw [N] or None, all fp32 -> float64 want and bound of dsig [N, 2T] and
    drgb [N, 2T, 3], the live-ray mask and the fp32 e and one of every sample (derivation (A))."""
    z, sig, nears, fars = z.float(), sig.float(), nears.float(), fars.float()
    d = torch.empty_like(z)
    d[:, :-1] = z[:, 1:] - z[:, :-1]
    d[:, -1] = (fars - nears) / torch.tensor(float(T), dtype=torch.float32)
    x = (-d) * sig
    e = torch.exp(x.double()).float()
    a = 1.0 - e
    one = (1.0 - a) + torch.tensor(EPS15, dtype=torch.float32)
    d, e, a, one = d.double(), e.double(), a.double(), one.double()
    sat = e < 2.0 ** -26
    d_e = 1.5 * _ulp32(e) + TINY
    d_a = torch.where(sat, torch.zeros_like(e), d_e + torch.where(e < 0.5, U24, 0.0))
    d_one = d_a
    lo, hi = (one - d_one).clamp(min=EPS15), one + d_one
    excl = _excl_prod(one)
    tr = excl.float().double()
    d_tr = torch.maximum(_excl_prod(hi) - excl, excl - _excl_prod(lo)) + U24 * tr + TINY
    w = (a * tr).float().double()
    d_w = a * d_tr + tr * d_a + U24 * w.abs() + TINY
    gi64, c = gi.double(), rgb.double()
    gw64 = gw.double() if gw is not None else torch.zeros(z.shape[0], dtype=torch.float64)
    bg = f32(bg)
    av = (gi64[:, None, :] * c).sum(-1) - bg * gi64.sum(-1, keepdim=True) + gw64[:, None]
    A = (gi64.abs()[:, None, :] * c.abs()).sum(-1) + abs(bg) * gi64.abs().sum(-1, keepdim=True) + gw64.abs()[:, None]
    d_av = 10 * U24 * A
    t = av * w
    d_t = av.abs() * d_w + w.abs() * d_av
    after, d_after = _suffix_excl(t), _suffix_excl(d_t)
    q = after / one
    d_q = d_after / lo + after.abs() * d_one / (one * lo)
    da = av * tr - q
    d_da = tr * d_av + av.abs() * d_tr + d_q + U24 * q.abs() + 2 * U24 * ((av * tr).abs() + q.abs()) + 3 * TINY
    dsig = da * d * e
    d_dsig = (d * e).abs() * d_da + (da * d).abs() * d_e + 2 * U24 * dsig.abs() + 2 * TINY
    drgb = w[..., None] * gi64[:, None, :]
    d_drgb = gi64.abs()[:, None, :] * d_w[..., None] + U24 * drgb.abs() + TINY
    return dict(dsig=dsig, dsig_bound=d_dsig, drgb=drgb, drgb_bound=d_drgb, mask=nears < fars, e=e, one=one)


def check_elements(name, got, want, bound, mask=None, lines=None):
    """Every (unmasked) element inside its bound; prints and returns the margin line.  Non-vacuity: some |want| > 0."""
    g = got.double().reshape(want.shape)
    if mask is not None:
        g, want, bound = g[mask], want[mask], bound[mask]
    assert bool(torch.isfinite(g).all()), f"{name}: output not finite"
    assert bool(torch.isfinite(bound).all()) and bool(torch.isfinite(want).all()), f"{name}: reference not finite"
    assert float(want.abs().max()) > 0, f"{name}: the reference is all zero"
    err = (g - want).abs()
    bad = err > bound
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    worst = int(ratio.argmax())
    nz = want != 0
    loosest = float((bound[nz] / want[nz].abs()).max())
    rel = float((g - want).norm() / want.norm())
    line = (f"margin {name}: worst err/bound {float(ratio.reshape(-1)[worst]):.3f} rel L2 vs float64 {rel:.2e} "
            f"median bound/max|want| {float(bound.median() / want.abs().max()):.2e} largest bound/|want| {loosest:.2e}")
    print(line)
    if lines is not None:
        lines.append(line)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {err.numel()} elements outside their bound; worst err / bound "
                                 f"{float(ratio.reshape(-1)[worst]):.3g} (got {float(g.reshape(-1)[worst]):.9g} want {float(want.reshape(-1)[worst]):.9g} "
                                 f"bound {float(bound.reshape(-1)[worst]):.3g}) at flat index {worst} of shape {tuple(want.shape)}")
    return line


def opaque_conditions(ref):
    """The three conditions on the opaque case, from the reference alone: (share of live samples with e in [1e-6, 1e-2], share with one == 1e-15f,
    share of live elements whose bound is at most 1e-4 of their ray's largest |want|, the smaller of d(sigma)'s and d(rgb)'s)."""
    m = ref["mask"]
    e, one = ref["e"][m], ref["one"][m]
    semi = float(((e >= 1e-6) & (e <= 1e-2)).double().mean())
    sat = float((one == EPS15).double().mean())
    ds, db = ref["dsig"][m], ref["dsig_bound"][m]
    dr, rb = ref["drgb"][m].flatten(1), ref["drgb_bound"][m].flatten(1)
    tight = lambda want, bound: float((bound <= 1e-4 * want.abs().max(1, keepdim=True).values).double().mean())
    return semi, sat, min(tight(ds, db), tight(dr, rb))                # the condition holds for d(sigma) and for d(rgb) on its own


# ---------------------------------------------------------------------------------------------------------------------------------
def sample_points(o, d, z, aabb, bound):
    """ngp_point + ngp_unit in fp32, as the kernel: x [N, M, 3] clipped to the box and whether the unit-box image lies in [0, 1]."""
    x = o.float()[:, None, :] + d.float()[:, None, :] * z.float()[:, :, None]
    x = torch.minimum(torch.maximum(x, aabb[:3].float()), aabb[3:].float())
    b = torch.tensor(float(bound), dtype=torch.float32)
    x01 = (x + b) / (2.0 * b)
    inside = ((x01 >= 0) & (x01 <= 1)).all(-1)
    return x, inside


def _backward64(dout, d_dout, m1, m2, w0, w1, w2):
    """dout, d_dout [..., 4]; masks [..., 64] (float64 0 / 1) -> dh2, d_dh2, dh1, d_dh1, dfeat, d_dfeat (derivation (B))."""
    dh2 = (dout @ w2) * m2
    e2 = (4 * U24 * (dout.abs() @ w2.abs()) + (d_dout + TINY) @ w2.abs() + TINY) * m2       # (TINY: a subnormal operand or result)
    dh1 = (dh2 @ w1) * m1
    e1 = (K2 * U24 * (dh2.abs() @ w1.abs()) + (e2 + TINY) @ w1.abs() + TINY) * m1
    df = dh1 @ w0
    edf = K2 * U24 * (dh1.abs() @ w0.abs()) + (e1 + TINY) @ w0.abs() + TINY
    return dh2, e2, dh1, e1, df, edf


def field_forward64(F, W, x, dsig, drgb):
    """Per-point forward and d(out) with their uncertainties; F [P, 32], W = (w0, b0, w1, b1, w2, b2), x [P, 3], dsig [P], drgb [P, 3]: fp32."""
    w0, b0, w1, b1, w2, b2 = (t.double() for t in W)
    F = F.double()
    z1 = F @ w0.T + b0
    m1 = (K1 + 2) * U24 * (F.abs() @ w0.abs().T + b0.abs())
    amb1 = z1.abs() <= m1
    h1 = z1.clamp(min=0)
    d_h1 = torch.where((z1 > 0) | amb1, m1, torch.zeros_like(m1))
    z2 = h1 @ w1.T + b1
    m2 = (K2 + 2) * U24 * (h1 @ w1.abs().T + b1.abs()) + d_h1 @ w1.abs().T
    amb2 = z2.abs() <= m2
    h2 = z2.clamp(min=0)
    d_h2 = torch.where((z2 > 0) | amb2, m2, torch.zeros_like(m2))
    out = h2 @ w2.T + b2
    d_out = (K2 + 2) * U24 * (h2 @ w2.abs().T + b2.abs()) + d_h2 @ w2.abs().T
    x = x.double()
    r2 = (x * x).sum(-1)
    blob = 5.0 * torch.exp(-r2 / C008)
    d_blob = blob * ((6 * r2 / C008 + 4) * U24)
    pre = out[:, 0] + blob
    d_pre = d_out[:, 0] + d_blob + U24 * pre.abs()
    dout0 = dsig.double() * torch.exp(pre.clamp(-15.0, 15.0))
    d_dout0 = dout0.abs() * (d_pre + 3 * U24)
    sg = torch.sigmoid(out[:, 1:])
    s1 = 1.0 - sg
    d_sg = 4 * U24 * sg + sg * s1 * d_out[:, 1:]
    d_s1 = d_sg + U24 * s1
    g = drgb.double()
    doutc = g * sg * s1
    d_doutc = g.abs() * (s1 * d_sg + sg * d_s1 + 2 * U24 * sg * s1)
    return dict(F=F, z1=z1, m1=m1, amb1=amb1, h1=h1, d_h1=d_h1, z2=z2, m2=m2, amb2=amb2, h2=h2, d_h2=d_h2, out=out, d_out=d_out,
                dout=torch.cat([dout0[:, None], doutc], 1), d_dout=torch.cat([d_dout0[:, None], d_doutc], 1))


def ambiguity(fw):
    """Ambiguous units per point, and the shares the conditions cap (reference alone)."""
    k = fw["amb1"].sum(1) + fw["amb2"].sum(1)
    P = k.numel()
    return k, int(((k > 0) & (k <= MAX_AMBIGUOUS)).sum()), int((k > MAX_AMBIGUOUS).sum()), P


def field_backward_check(name, fw, W, inside, got_dfeat, lines=None):
    """The per-point backward of derivation (B) against the kernel's d(feat) rows got_dfeat [P, 32]: resolves the ambiguous points' masks,
    asserts every checked row, and returns what the weight gradients need (dh2, dh1 with their uncertainties) and the counts."""
    w0, _, w1, _, w2, _ = (t.double() for t in W)
    ins = inside.double()[:, None]
    base1, base2 = (fw["z1"] > 0).double(), (fw["z2"] > 0).double()
    dh2, e2, dh1, e1, df, edf = _backward64(fw["dout"], fw["d_dout"], base1, base2, w0, w1, w2)
    k, n_amb, n_left, P = ambiguity(fw)
    got = got_dfeat.double()
    extra2, extra1 = torch.zeros_like(dh2), torch.zeros_like(dh1)
    dh2_base, dh1_base = dh2.clone(), dh1.clone()                      # with the masks of the float64 signs
    inferred = 0
    A = torch.nonzero((k > 0) & (k <= MAX_AMBIGUOUS)).flatten()
    if A.numel():
        amb = torch.cat([fw["amb1"][A], fw["amb2"][A]], 1)                           # [nA, 128]
        rank = (amb.long().cumsum(1) - 1).clamp(min=0)
        C = 1 << MAX_AMBIGUOUS
        bits = ((torch.arange(C)[None, :, None] >> rank[:, None, :]) & 1).double()
        base = torch.cat([base1[A], base2[A]], 1)
        cand = torch.where(amb[:, None, :], bits, base[:, None, :].expand(-1, C, -1))
        valid = torch.arange(C)[None, :] < (1 << k[A])[:, None]
        c2, ce2, c1, ce1, cdf, cedf = _backward64(fw["dout"][A][:, None, :], fw["d_dout"][A][:, None, :], cand[..., :64], cand[..., 64:], w0, w1, w2)
        cdf, cedf = cdf * ins[A][:, None, :], cedf * ins[A][:, None, :]
        err = (got[A][:, None, :] - cdf).abs()
        fit = (err <= cedf).all(-1) & valid
        score = torch.where(err > 0, err / cedf.clamp(min=1e-300), torch.zeros_like(err)).max(-1).values
        score = torch.where(valid, score, torch.full_like(score, float("inf")))
        ch = score.argmin(1)
        base_idx = (amb.long() * base.long() * (1 << rank)).sum(1)                     # the candidate with the float64 signs wins a tie
        rows = torch.arange(A.numel())
        ch = torch.where(score[rows, base_idx] <= score[rows, ch], base_idx, ch)
        pick = lambda t: t[torch.arange(A.numel()), ch]
        inferred = int((pick(cand) != base).any(-1).sum())
        others = fit[..., None].double()
        extra2[A] = ((c2 - pick(c2)[:, None, :]).abs() * others).max(1).values
        extra1[A] = ((c1 - pick(c1)[:, None, :]).abs() * others).max(1).values
        dh2[A], e2[A], dh1[A], e1[A], df[A], edf[A] = pick(c2), pick(ce2), pick(c1), pick(ce1), pick(cdf), pick(cedf)
    df, edf = df * ins, edf * ins
    left = k > MAX_AMBIGUOUS
    if bool(left.any()):
        a2 = fw["dout"][left].abs() @ w2.abs()
        extra2[left], extra1[left] = a2, a2 @ w1.abs()
    check_elements(f"{name} d(feat)", got, df, edf, mask=~left[:, None].expand(-1, df.shape[1]), lines=lines)
    return dict(dh2=dh2, d_dh2=e2 + extra2, dh1=dh1, d_dh1=e1 + extra1, dfeat=df, dfeat_bound=edf, ambiguous=n_amb, left_out=n_left,
                inferred=inferred, points=P, dh2_base=dh2_base, dh1_base=dh1_base)


def flip_effect(fw, bk):
    """Relative L2 by which the inferred masks (those that differ from the float64 signs) move dW0, db0, dW1, db1."""
    d2, d1 = bk["dh2"] - bk["dh2_base"], bk["dh1"] - bk["dh1_base"]
    rel = lambda d, full: float(d.norm() / full.norm())
    return dict(w0=rel(d1.T @ fw["F"], bk["dh1"].T @ fw["F"]), b0=rel(d1.sum(0), bk["dh1"].sum(0)),
                w1=rel(d2.T @ fw["h1"], bk["dh2"].T @ fw["h1"]), b1=rel(d2.sum(0), bk["dh2"].sum(0)))


def _wave_sums(pairs, geo, block=512):
    """sum over pairs (A [P, a], B [P, b]) of A^T B restricted to every wave's points -> [n_waves, a, b]."""
    a, b = pairs[0][0].shape[1], pairs[0][1].shape[1]
    out = torch.zeros(geo["n_waves"], a, b, dtype=torch.float64)
    for p0, P, trips, _ in geo["chunks"]:
        pad = trips * FB_PTS - P
        wave_of_trip = geo["wave"][p0:p0 + P:FB_PTS]
        tile = lambda t: torch.cat([t[p0:p0 + P], torch.zeros(pad, t.shape[1], dtype=torch.float64)]).view(trips, FB_PTS, -1)
        As = torch.cat([tile(A) for A, _ in pairs], 1)
        Bs = torch.cat([tile(B) for _, B in pairs], 1)
        for t0 in range(0, trips, block):
            out.index_add_(0, wave_of_trip[t0:t0 + block], As[t0:t0 + block].transpose(1, 2) @ Bs[t0:t0 + block])
    return out


def weight_grads_ref64(fw, bk, geo):
    """The six weight / bias gradients as float64 sums with their per-element bounds (derivation (B)): name -> (want, bound, waves on the fp32
    path per element).  fw = field_forward64(...), bk = field_backward_check(...), geo = bwd_geometry(...)."""
    P = fw["F"].shape[0]
    assert P == geo["wave"].numel()
    co = geo["coef"][:, None]
    one, F = torch.ones(P, 1, dtype=torch.float64), fw["F"]
    zero = torch.zeros(P, 1, dtype=torch.float64)
    # (left factor, its uncertainty, right factor, its uncertainty)
    terms = {"w0": (bk["dh1"], bk["d_dh1"], F, torch.zeros_like(F)), "b0": (bk["dh1"], bk["d_dh1"], one, zero),
             "w1": (bk["dh2"], bk["d_dh2"], fw["h1"], fw["d_h1"]), "b1": (bk["dh2"], bk["d_dh2"], one, zero),
             "w2": (fw["dout"], fw["d_dout"], fw["h2"], fw["d_h2"]), "b2": (fw["dout"], fw["d_dout"], one, zero)}
    n_flush = sum(4 * grid for _, _, _, grid in geo["chunks"])
    thr = geo["thr"]
    out = {}
    for name, (L, dL, R, dR) in terms.items():
        S = _wave_sums([(L, R)], geo)
        E = _wave_sums([(co * L.abs(), R.abs()), (dL + TINY, R.abs()), (L.abs(), dR + TINY)], geo)
        want = S.sum(0)
        big = S.abs() + E >= thr                                      # waves that may take the fp32 atomic
        kb = big.sum(0).double()
        chain = kb * U24 * ((S.abs() + E) * big).sum(0)
        bound = E.sum(0) + n_flush * 2.0 ** -45 + chain + P * TINY
        bound = bound + torch.where(kb > 0, 3.0, 1.0) * U24 * (want.abs() + bound)
        sure = (S.abs() - E >= thr).sum(0)
        if R is one:
            want, bound, kb, sure = want[:, 0], bound[:, 0], kb[:, 0], sure[:, 0]
        out[name] = dict(want=want, bound=bound, maybe_fp32=kb, sure_fp32=sure, sum_abs=(L.abs().T @ R.abs()).reshape(want.shape),
                         max_wave_sum=float(S.abs().max()))
    return out


def opaque_sigma(z, nears, fars, T, seed):
    """A synthetic sigma for sorted depths z [N, 2T] that drives stage A through all three regimes: every ray is almost transparent up to a
    random position (d sigma <= 0.5: thinner samples leave d(sigma) so small that the worst-case bound of
    the 2T alphas in front exceeds 1e-4 of it), then crosses three semi-opaque samples (e = exp(-d sigma) between 1e-6 and 1e-2), and behind them every
    third sample on average is saturated (d sigma in [20, 60]: e < 2^-26, one == 1e-15f) and every sixth semi-opaque, between transparent ones."""
    g = torch.Generator().manual_seed(seed)
    N, M = z.shape
    d = torch.empty_like(z)
    d[:, :-1] = z[:, 1:] - z[:, :-1]
    d[:, -1] = (fars - nears) / float(T)
    pos = torch.arange(M)[None, :]
    s0 = torch.randint(0, M - 3, (N, 1), generator=g)
    u = torch.rand(N, M, generator=g)
    thin = 0.5 * u
    semi = 4.7 + (13.7 - 4.7) * u
    thick = 20.0 + 40.0 * u
    u2 = torch.rand(N, M, generator=g)
    behind = torch.where(u2 < 1.0 / 3.0, thick, torch.where(u2 < 0.5, semi, thin))
    target = torch.where(pos < s0, thin, torch.where(pos < s0 + 3, semi, behind))
    return torch.where(d > 0, target / d.clamp(min=1e-30), torch.zeros_like(d)).float().contiguous()

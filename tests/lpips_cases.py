"""Shared cases of the perceptual-loss kernels and plans (sparsefusion_amd/csrc/lpips_kernels.h, sparsefusion_amd/lpips.py).

Part A -- the eight small kernels, one op at a time: the same op descriptors run either on CPU fibers (backend "emu": tests/hostemu/lpips_emu.cpp,
the kernel source without a GPU) or through the C ABI on the GPU (backend "gpu": sf_plan_run).  Every destination is prefilled with a
sentinel and sits between two guard bands, so an element that was never written and a write outside the logical extent both show.
Part B -- every launch of the LPIPS forward and backward plans, stepped one op at a time (run_plan_case): the op's operand and destination
buffers are decoded from the op record alone, copied to the host, and the launch's result is compared with the float64 evaluation of that op
ON THE VALUES IT ACTUALLY READ -- no error is carried from one launch to the next, so each op's bound is that of a single launch.

Expectations are exact (bit for bit / torch.equal) for max pooling, ReLU backward, the eltwise add, the fixed-point -> float conversion and
the operand-type twins.  Everywhere else every element has a bound, derived below by counting the roundings of the kernel's longest chain.
No constant of it is fitted to a kernel's output; the measured margins are in profiles/lpips_op_parity_margins.log.

The bounds.  u = 2^-24 is the unit roundoff of fp32 round-to-nearest; every term is first order in u.  The library is compiled without fast-math
flags, and hipcc then evaluates `/` and sqrtf correctly rounded: 1 u each (U_DIV, U_SQRT; a hardware approximation would be 2 u).  A sum of n
fp32 additions (an fma counts as one) is off by at most n u sum|terms|; a contraction of a * b + c into an fma only removes a rounding.

(a) the scaling layer  (x - shift) / scale: the subtraction (1 u of |x - shift|, which is the quotient's relative error too) and the division:
    (1 + U_DIV) u |want|.  Its gradient g / scale: U_DIV u |want|.  Padded channels: exactly 0.
(b) the head, per pixel (one wave; lane l holds channels 4 l .. 4 l + 3 of each 256-channel trip, T = ceil(C / 256) <= 2 trips):
    n = sum_c f_c^2: a square is rounded (1), added inside its float4 (<= 3), into the lane's sum (<= T = 2 more trips), through 6 shuffle
      levels: N_NORM = 12 roundings on any term; all terms are positive, so n is off by N_NORM u n and |f| = sqrt(n) by (N_NORM / 2 + U_SQRT) u |f|;
    r = 1 / (|f| + eps): the add (1; eps is positive and exact) and the division:  rho = N_NORM / 2 + U_SQRT + 1 + U_DIV  (relative, in u);
    e_c = a_c r0 - b_c r1 = u_c - v_c: two products (rho + 1 each) and the subtraction (1 u of at most |u_c| + |v_c|):
      d(e_c) = (rho + 2) u (|u_c| + |v_c|)   -- u_c and v_c cancel, so the rounding acts on their magnitudes, not on e_c;
    forward:  t_c = w_c e_c^2 through fmaf(w e, e, d): d(t_c) = 2 w_c |e_c| d(e_c) + u w_c e_c^2; the lane's fma chain (4 T <= 8) and 6 shuffle
      levels: N_D = 14 roundings on the (non-negative) pixel sum.  A wave adds its P = ceil(HW / (4 * workgroups per sample)) pixels (P), the
      four waves meet (3), the division by HW (U_DIV), one rounding to the 2^-44 grid per WORKGROUP (absolute, 2^-44 each: FIX), and the
      conversion of the integer total to float (1):
        bound(D_s) = mean_p sum_c d(t_c)  +  (N_D + P + 3 + U_DIV + 1) u D_s  +  workgroups * 2^-44.
      The increment of the fixed-point accumulator by ONE head launch (Part B) carries everything but the last rounding.
    backward:  A_c = 2 w_c e_c (2 w exact, one product):  d(A_c) = 2 w_c d(e_c) + u |A_c|;
      dot = sum_c A_c a_c (fma chain + shuffles):  d(dot) = sum_c |a_c| d(A_c) + N_D u sum_c |A_c a_c|;
      k2 = dot r0 r0 / |f0| (0 for an all-zero pixel):  d(k2) = r0^2 / |f0| d(dot) + |k2| (2 rho + N_NORM / 2 + U_SQRT + 2 + U_DIV) u;
      g = gscale / HW: U_DIV u |g|;   out_c = g (A_c r0 - a_c k2).  The two terms t1 = A_c r0 and t2 = a_c k2 cancel (the gradient is
      tangential), so the roundings of the subtraction (1), of the product with g (1) and of g (U_DIV) act on |t1| + |t2|:
        bound(out_c) = |g| ( r0 d(A_c) + |t1| (rho + 1) u  +  |a_c| d(k2) + u |t2|  +  (2 + U_DIV) u (|t1| + |t2|) ).
      For a pixel whose f0 is all zero autograd gives NaN; the kernel documents the one-sided limit out_c = g 2 w_c (0 - v_c) / (0 + eps),
      which is what the closed form above gives with a = 0 (k2 = 0), and the same bound holds.
(c) a convolution: operands of the operand type (bf16 / IEEE half) have exact products in fp32; the roundings are the fp32 additions.
    The per-element bound is  c u conv(|a|, |w|)  +  n_epi u (|conv| + |bias| + |previous|),  n_epi = the epilogue adds (bias, accumulate), with c
    the number of additions on the longest accumulation chain of the kernel family the op's `tile` field selects:
      k_conv_igemm (tile < 256): clause (b) of tests/fused_cases.py:  c = ceil(K / (128 S)) + 32 + 8 + S  (S split-K groups: the chain of a wave's
        MFMAs, <= 32 additions inside one MFMA, the 4-wave K-slice reduction in LDS counted as 8, the slab sum);
      the LDS-tiled kernels (tile >= 256: k_conv_lds, k_conv_glds, k_conv3_halo, k_conv3_halo_sm; csrc/conv_lds_body.inc, conv_glds.h,
        conv_halo.h, conv_halo_small.h): each of the 4 (8) matrix waves owns whole output fragments and runs the WHOLE K range through one
        accumulator -- K / 32 chained MFMAs of <= 32 additions each, in tap-major or chunk-major order; no K-slice reduction:
        c = ceil(K / (32 S)) + 32 + S  (S = 1 in every LPIPS plan).
    The condition on the reference alone (asserted): median(bound) / rms(want) <= BOUND_MEDIAN_MAX = 1e-3 -- a looser bound hides errors."""
import math

import torch
import torch.nn.functional as F

from hostemu import lpips_emu
from oracle import lpips_ref
from sparsefusion_amd import _lib

OP_CONV, OP_ELTWISE, OP_MEMSET, OP_POOL, OP_LPIPS = 1, 7, 8, 11, 12
U24, FIX = 2.0 ** -24, 2.0 ** -44
U_DIV, U_SQRT = 1, 1
N_NORM, N_D = 12, 14
RHO = N_NORM / 2 + U_SQRT + 1 + U_DIV
EPS = float(torch.tensor(1e-10, dtype=torch.float32))          # LPIPS_EPS as the kernel holds it
BOUND_MEDIAN_MAX, TAP_NONZERO_MIN, DIST_MIN = 1e-3, 0.25, 1e-3    # conditions of the reference alone (asserted)
GUARD, SENTINEL = 64, 12345.6789
_KEEP = []


def device_of(backend):
    return "cpu" if backend in ("emu", "ref") else "cuda:0"


def mkop(type_, flags=0, p=(), i=()):
    o = _lib.SfOp()
    o.type, o.flags = type_, flags
    for k, v in enumerate(p):
        if torch.is_tensor(v):
            _KEEP.append(v)
        o.p[k] = (v.data_ptr() if torch.is_tensor(v) else v) or None
    for k, v in enumerate(i):
        o.i[k] = int(v)
    return o


def run_ops(ops, backend, operand=None):
    """operand: None = the process library (bf16 under emulation), "bf16" | "f16" = that operand build"""
    if backend == "emu":
        lpips_emu.run(ops, operand or "bf16")
    else:
        lib = _lib.lib(operand)
        arr = (_lib.SfOp * len(ops))(*ops)
        _lib.check(lib.sf_plan_run(arr, len(ops), _lib.stream_ptr()), "plan", lib)
        torch.cuda.synchronize()
    del _KEEP[:]


def opnd_dtype(backend, operand=None):
    if backend == "emu":
        return torch.float16 if operand == "f16" else torch.bfloat16
    return _lib.operand_dtype(_lib.lib(operand))


def guarded(n, dtype, dev, fill=SENTINEL):
    """(whole buffer, its n-element body): GUARD elements on either side; everything holds the sentinel"""
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return t, t[GUARD:GUARD + n]


def guards_intact(t, fill=SENTINEL):
    ref = torch.full((GUARD,), fill, dtype=t.dtype)
    return torch.equal(t[:GUARD].cpu(), ref) and torch.equal(t[-GUARD:].cpu(), ref)


def worst(what, got, want, bound):
    """|got - want| <= bound for every element -> (worst err / bound, None or a failure report)"""
    got, want, bound = got.double().reshape(-1), want.double().reshape(-1), bound.double().reshape(-1)
    err = (got - want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    k = int(ratio.argmax()) if ratio.numel() else 0
    bad = int((err > bound).sum())
    msg = None if bad == 0 else (f"{what}: {bad} of {err.numel()} elements outside their bound; worst err / bound {float(ratio[k]):.3g} at flat index {k}: "
                                 f"got {float(got[k])!r} want {float(want[k])!r} bound {float(bound[k]):.3g}")
    return (float(ratio[k]) if ratio.numel() else 0.0), msg


# ---------------------------------------------------------------------------------------------------------------------------------
# max pooling
POOL_SHAPES = [(1, 2, 2, 4), (3, 6, 10, 64), (2, 16, 16, 512)]      # (B, H, W, C): the smallest legal; non-square, work % 256 != 0; two full grids of float4
_POOL_EXTRA = ["eq4", "tie12", "tie03", "tie23", "zero", "signed_zero_a", "signed_zero_b"]
POOL_PATTERNS = [f"max{k}" for k in range(4)] + _POOL_EXTRA          # each of them in each of the four channel lanes of a float4


def _pool_window(pattern, base):
    """the four values (row-major) of a planted window; base: four distinct random values in (-2, 1)"""
    v = base.clone()
    if pattern.startswith("max"):
        v[int(pattern[3])] = 5.0
    elif pattern == "eq4":
        v[:] = 1.25
    elif pattern.startswith("tie"):
        v[int(pattern[3])] = v[int(pattern[4])] = 2.5
    elif pattern == "zero":
        v[:] = 0.0
    elif pattern == "signed_zero_a":
        v = torch.tensor([-0.0, 0.0, -0.0, 0.0])
    else:
        v = torch.tensor([0.0, -0.0, -0.0, -0.0])
    return v


def pool_input(B, H, W, C, rep, seed=0):
    """NHWC input with planted windows: slot n of channel lane l (window n // (C / 4) in (b, oy, ox) order, channel 4 (n % (C / 4)) + l)
    holds pattern rep * slots + n of POOL_PATTERNS while that index exists.  -> x, number of windows planted"""
    g = torch.Generator().manual_seed(seed + 17 * rep)
    x = torch.rand(B, H, W, C, generator=g) * 3 - 2
    Ho, Wo, c4 = H // 2, W // 2, C // 4
    slots = B * Ho * Wo * c4
    planted = 0
    for lane in range(4):
        for n in range(min(slots, len(POOL_PATTERNS))):
            j = rep * slots + n
            if j >= len(POOL_PATTERNS):
                break
            wdx, c = n // c4, 4 * (n % c4) + lane
            b, oy, ox = wdx // (Ho * Wo), wdx // Wo % Ho, wdx % Wo
            v = _pool_window(POOL_PATTERNS[j], x[b, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2, c].reshape(4))
            x[b, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2, c] = v.view(2, 2)
            planted += 1
    return x, planted


def pool_reps(B, H, W, C):
    slots = B * (H // 2) * (W // 2) * (C // 4)
    return max(1, math.ceil(len(POOL_PATTERNS) / slots))


def pool_expected(x, dout):
    """torch on the CPU: forward, and the autograd of F.max_pool2d (first maximum in row-major order, signed zeros and all-equal windows too)"""
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.max_pool2d(xn, 2)
    y.backward(dout.permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).contiguous(), xn.grad.permute(0, 2, 3, 1).contiguous()


def run_pool_case(backend, B, H, W, C):
    dev = device_of(backend)
    planted = 0
    for rep in range(pool_reps(B, H, W, C)):
        x, n = pool_input(B, H, W, C, rep)
        planted += n
        g = torch.Generator().manual_seed(5 + rep)
        dout = (torch.rand(B, H // 2, W // 2, C, generator=g) + 0.5) * (torch.randint(0, 2, (B, H // 2, W // 2, C), generator=g) * 2 - 1)
        want_y, want_dx = pool_expected(x, dout)
        xd, dd = x.to(dev), dout.to(dev)
        ybuf, y = guarded(want_y.numel(), torch.float32, dev)
        gbuf, dx = guarded(x.numel(), torch.float32, dev)
        run_ops([mkop(OP_POOL, 0, p=(xd, None, None, y), i=(B, H, W, C)),
                 mkop(OP_POOL, 1, p=(dd, xd, None, dx), i=(B, H, W, C))], backend)
        assert guards_intact(ybuf) and guards_intact(gbuf), "pool: a write outside the tensor"
        assert torch.equal(y.cpu().view(want_y.shape), want_y), "pool forward differs from F.max_pool2d"
        got = dx.cpu().view(x.shape)
        assert torch.equal(got, want_dx), f"pool backward differs from the autograd of F.max_pool2d at {int((got != want_dx).sum())} elements"
        assert int((got != 0).sum()) == want_y.numel()          # one routed gradient per window and channel, exact zeros everywhere else
    assert planted == 4 * len(POOL_PATTERNS)                    # every pattern in every channel lane
    print(f"pool ({B}, {H}, {W}, {C}): forward and backward equal torch; {planted} planted windows")


# ---------------------------------------------------------------------------------------------------------------------------------
# the heads
HEAD_SHAPES = [(1, 1, 64), (2, 5, 128), (3, 64, 256), (2, 16, 512), (1, 1100, 512)]      # (V, HW, C): see tests/test_gpu_lpips_ops.py
HEAD_PLANTS = ("f0_zero", "f1_zero", "both_zero")


def head_feats(V, HW, C, plant, seed):
    """[2V, HW, C] non-negative, about half zeros; plant: which of HEAD_PLANTS to put, in pixels 0, 1, 2 of the flat (sample, pixel) order
    (a shape with fewer than 4 pixels takes one plant per call, in pixel 0)"""
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(2 * V, HW, C, generator=g))
    assert 0.35 < float((f == 0).double().mean()) < 0.65
    for q, kind in enumerate(plant):
        s, p = q // HW, q % HW
        if kind in ("f0_zero", "both_zero"):
            f[s, p] = 0
        if kind in ("f1_zero", "both_zero"):
            f[V + s, p] = 0
    w = torch.rand(C, generator=g) / C * 4
    return f, w


def head_plants(V, HW):
    return [HEAD_PLANTS] if V * HW >= 4 else [()] + [(k,) for k in HEAD_PLANTS]


def head_workgroups(HW):
    """(workgroups per sample, pixels per wave) of k_lpips_head_fwd's launch (lpips_launch_of)"""
    per = min((HW + 3) // 4, 256)
    return per, math.ceil(HW / (4 * per))


def head_terms64(feats, w, V):
    """the float64 quantities of the header comment's formula, and d(e_c) of derivation (b)"""
    f = feats.double()
    f0, f1, w = f[:V], f[V:], w.double()
    l0, l1 = (f0 * f0).sum(-1, keepdim=True).sqrt(), (f1 * f1).sum(-1, keepdim=True).sqrt()
    r0, r1 = 1.0 / (l0 + EPS), 1.0 / (l1 + EPS)
    u, v = f0 * r0, f1 * r1
    e = u - v
    return dict(f0=f0, w=w, l0=l0, r0=r0, e=e, de=(RHO + 2) * U24 * (u.abs() + v.abs()), d=(w * e * e).sum(-1))


def head_forward64(feats, w, V, final=True):
    """-> float64 distance per sample [V], its bound; final=False: the increment of the fixed-point accumulator (no conversion to float)"""
    t = head_terms64(feats, w, V)
    HW = feats.shape[1]
    per, ppw = head_workgroups(HW)
    dt = 2 * t["w"] * t["e"].abs() * t["de"] + U24 * t["w"] * t["e"] * t["e"]
    D = t["d"].mean(1)
    return D, dt.sum(-1).mean(1) + (N_D + ppw + 3 + U_DIV + (1 if final else 0)) * U24 * D + per * FIX


def head_autograd64(feats, w, V, gscale):
    """float64 autograd of the float64 forward: d (sum_s gscale_s D_s) / d f0 (NaN where f0 is all zero)"""
    f = feats.double()
    f0 = f[:V].clone().requires_grad_(True)
    f1, w = f[V:], w.double()
    n0, n1 = (f0 * f0).sum(-1, keepdim=True).sqrt(), (f1 * f1).sum(-1, keepdim=True).sqrt()
    e = f0 / (n0 + EPS) - f1 / (n1 + EPS)
    ((w * e * e).sum(-1).mean(1) * gscale.double()).sum().backward()
    return f0.grad


def head_backward64(feats, w, V, gscale):
    """-> want [V, HW, C] (autograd where |f0| > 0, the documented one-sided limit where f0 is all zero), bound"""
    t = head_terms64(feats, w, V)
    HW = feats.shape[1]
    f0, wt, e, de, l0, r0 = t["f0"], t["w"], t["e"], t["de"], t["l0"], t["r0"]
    A = 2 * wt * e
    dA = 2 * wt * de + U24 * A.abs()
    dot = (A * f0).sum(-1, keepdim=True)
    ddot = (f0.abs() * dA).sum(-1, keepdim=True) + N_D * U24 * (A * f0).abs().sum(-1, keepdim=True)
    live = l0 > 0
    l0s = torch.where(live, l0, torch.ones_like(l0))
    k2 = torch.where(live, dot * r0 * r0 / l0s, torch.zeros_like(dot))
    dk2 = torch.where(live, r0 * r0 / l0s * ddot + k2.abs() * (2 * RHO + N_NORM / 2 + U_SQRT + 2 + U_DIV) * U24, torch.zeros_like(dot))
    g = (gscale.double() / HW).view(V, 1, 1)
    t1, t2 = A * r0, f0 * k2
    closed = g * (t1 - t2)
    bound = g.abs() * (r0 * dA + t1.abs() * (RHO + 1) * U24 + f0.abs() * dk2 + U24 * t2.abs() + (2 + U_DIV) * U24 * (t1.abs() + t2.abs()))
    auto = head_autograd64(feats, w, V, gscale)
    lv = live.expand_as(auto)
    if bool(lv.any()):          # the closed form the bound is built on IS the autograd gradient (reference against reference)
        assert float((auto[lv] - closed[lv]).abs().max()) <= 1e-9 * float(closed[lv].abs().max()) + 1e-300
    want = torch.where(lv, auto, closed)
    assert bool(torch.isfinite(want).all())
    return want, bound


def _head_ops(fd, wd, acc, dist, V, HW, C):
    return mkop(OP_LPIPS, 0, p=(fd, wd, None, acc), i=(V, HW, C)), mkop(OP_LPIPS, 2, p=(None, None, acc, dist), i=(V, 0, 0))


def _acc(V, dev):
    buf, acc = guarded(V, torch.int64, dev, fill=0x5a5a5a5a5a5a)
    acc.zero_()
    return buf, acc


def run_head_fwd_case(backend, V, HW, C):
    dev = device_of(backend)
    top = 0.0
    for k, plant in enumerate(head_plants(V, HW)):
        f, w = head_feats(V, HW, C, plant, seed=V * 1000 + HW + k)
        want, bound = head_forward64(f, w, V)
        fd, wd = f.to(dev), w.to(dev)
        abuf, acc = _acc(V, dev)
        dbuf, dist = guarded(V, torch.float32, dev)
        run_ops(list(_head_ops(fd, wd, acc, dist, V, HW, C)), backend)
        assert guards_intact(abuf, 0x5a5a5a5a5a5a) and guards_intact(dbuf), "head forward: a write outside the accumulator / the distances"
        r, msg = worst(f"head forward ({V}, {HW}, {C}) plant {plant}", dist.cpu(), want, bound)
        assert msg is None, msg
        top = max(top, r)
        if k == 0:
            tight = float((bound / want).max())
    print(f"head forward ({V}, {HW}, {C}): worst err / bound {top:.3f}; bound / distance {tight:.2e}")


def run_head_pair_case(backend, shapes=((2, 16, 512), (2, 5, 128))):
    """two taps into ONE accumulator: the sum of their float64 references, and the same bits whichever head launch is issued first"""
    dev = device_of(backend)
    V = shapes[0][0]
    taps = []
    want, bound = torch.zeros(V, dtype=torch.float64), torch.zeros(V, dtype=torch.float64)
    for k, (v, HW, C) in enumerate(shapes):
        assert v == V
        f, w = head_feats(V, HW, C, HEAD_PLANTS, seed=77 + k)
        D, b = head_forward64(f, w, V)
        want, bound = want + D, bound + b
        taps.append((f.to(dev), w.to(dev), HW, C))
    bits = []
    for order in (taps, taps[::-1]):
        abuf, acc = _acc(V, dev)
        dbuf, dist = guarded(V, torch.float32, dev)
        ops = [_head_ops(fd, wd, acc, dist, V, HW, C)[0] for fd, wd, HW, C in order] + [mkop(OP_LPIPS, 2, p=(None, None, acc, dist), i=(V, 0, 0))]
        run_ops(ops, backend)
        assert guards_intact(abuf, 0x5a5a5a5a5a5a) and guards_intact(dbuf)
        r, msg = worst("two heads, one accumulator", dist.cpu(), want, bound)
        assert msg is None, msg
        bits.append((acc.cpu().tolist(), dist.cpu().view(torch.int32).tolist()))
    assert bits[0] == bits[1], f"the order of the head launches shows in the result: {bits}"
    print(f"two heads into one accumulator: worst err / bound {r:.3f}; both orders give the bits {bits[0][1]}")


def head_gscale(V, k=0):
    """differs per sample, with a negative value and a zero (one sample: one of them per call)"""
    return torch.tensor([[-0.7, 0.0, 1.3][(s + k) % 3] for s in range(V)])


def run_head_bwd_case(backend, V, HW, C):
    dev = device_of(backend)
    top = 0.0
    for k, plant in enumerate(head_plants(V, HW)):
        for gk in range(2 if V == 1 else 1):
            f, w = head_feats(V, HW, C, plant, seed=V * 1000 + HW + k)
            gs = head_gscale(V, gk)
            want, bound = head_backward64(f, w, V, gs)
            fd, wd, gd = f.to(dev), w.to(dev), gs.to(dev)
            obuf, out = guarded(V * HW * C, torch.float32, dev)
            run_ops([mkop(OP_LPIPS, 1, p=(fd, wd, gd, out), i=(V, HW, C))], backend)
            assert guards_intact(obuf), "head backward: a write outside the gradient"
            got = out.cpu().view(V, HW, C)
            assert bool(torch.isfinite(got).all()), "head backward: a non-finite gradient"
            r, msg = worst(f"head backward ({V}, {HW}, {C}) plant {plant} gscale {gs.tolist()}", got, want, bound)
            assert msg is None, msg
            top = max(top, r)
            if k == 0 and gk == 0:
                tight = float(bound.mean() / want.pow(2).mean().sqrt())
    print(f"head backward ({V}, {HW}, {C}): worst err / bound {top:.3f}; mean bound / rms {tight:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------------
# ReLU backward, the scaling layer
def relu_bwd_inputs(n, seed=3):
    """y with +0.0, -0.0, a positive denormal and negative values; dy with values that need rounding to either operand type: ties to even
    in both directions (the low 16 / 13 bits exactly half, the kept LSB 0 and 1), just below and above a tie, and -0.0"""
    g = torch.Generator().manual_seed(seed + n)
    y = torch.randn(n, generator=g)
    y[0], y[1], y[2], y[3] = 0.0, -0.0, 1e-40, -1.5
    dy = torch.randn(n, generator=g) * 3
    bits = dy.view(torch.int32).clone()
    for j in range(4, n):
        low, keep = [(0x8000, 16), (0x7fff, 16), (0x8001, 16), (0x1000, 13), (0x0fff, 13), (0x1001, 13)][j % 6]
        b = int(bits[j]) & ~((1 << keep) - 1)
        if (j // 6) % 2:
            b |= 1 << keep              # the kept LSB set: the tie rounds up; clear: it rounds down
        else:
            b &= ~(1 << keep)
        bits[j] = b | low
    dy = bits.view(torch.float32).clone()
    y[4:] = y[4:].abs() * (torch.arange(4, n) % 5 != 0)          # mostly positive, every fifth +0.0 ...
    y[7::11] = -y[7::11] - 0.25                                  # ... and some negative
    dy[0], dy[1], dy[2], dy[3] = 2.0, 3.0, -0.0, 4.0
    if n > 8:
        dy[8] = -0.0
        y[8] = 0.5
    return dy, y


def run_relu_bwd_case(backend, n, operand):
    dev = device_of(backend)
    dt = opnd_dtype(backend, operand)
    assert dt == (torch.float16 if operand == "f16" else torch.bfloat16)
    dy, y = relu_bwd_inputs(n)
    want = torch.where(y > 0, dy, torch.zeros_like(dy)).to(dt)
    obuf, out = guarded(n, torch.int16, dev, fill=0x5a5a)
    run_ops([mkop(OP_ELTWISE, 7, p=(dy.to(dev), y.to(dev), None, out), i=(n,))], backend, operand)
    assert guards_intact(obuf, 0x5a5a), "relu backward: a write outside the tensor"
    got = out.cpu()
    diff = got != want.view(torch.int16)
    assert not bool(diff.any()), (f"relu backward ({operand}): {int(diff.sum())} of {n} bit patterns differ, first at {int(diff.nonzero()[0])}: "
                                  f"dy {float(dy[diff][0])!r} y {float(y[diff][0])!r} got {int(got[diff][0]) & 0xffff:#06x} want {int(want.view(torch.int16)[diff][0]) & 0xffff:#06x}")
    assert int(want.view(torch.int16)[2]) & 0xffff == 0x8000 and float(want[1]) == 0        # -0.0 passes under a positive denormal; y = -0.0 masks
    print(f"relu backward n = {n} ({operand}): {n} bit patterns equal")


SCALE_SHAPES = [(1, 1, 32), (3, 35, 32)]


def scale_in64(x, k, Cp):
    """[B, 3, HW] -> want [B, HW, Cp], bound ((a) above)"""
    B, _, HW = x.shape
    k = k.double()
    want = torch.zeros(B, HW, Cp, dtype=torch.float64)
    want[:, :, :3] = ((x.double() - k[:3].view(1, 3, 1)) / k[3:].view(1, 3, 1)).permute(0, 2, 1)
    return want, (1 + U_DIV) * U24 * want.abs()


def scale_in_bwd64(g, k):
    """[B, HW, ld] -> want [B, 3, HW], bound"""
    want = (g.double()[:, :, :3] / k.double()[3:].view(1, 1, 3)).permute(0, 2, 1).contiguous()
    return want, U_DIV * U24 * want.abs()


def run_scale_case(backend, B, HW, Cp):
    dev = device_of(backend)
    g = torch.Generator().manual_seed(B * 100 + HW)
    x = torch.rand(B, 3, HW, generator=g) * 2 - 1
    k = torch.tensor(lpips_ref.SHIFT + lpips_ref.SCALE, dtype=torch.float32)
    want, bound = scale_in64(x, k, Cp)
    obuf, out = guarded(B * HW * Cp, torch.float32, dev)
    gr = torch.randn(B, HW, Cp, generator=g)
    want_b, bound_b = scale_in_bwd64(gr, k)
    bbuf, dx = guarded(B * 3 * HW, torch.float32, dev)
    run_ops([mkop(OP_ELTWISE, 8, p=(x.to(dev), k.to(dev), None, out), i=(B, HW, Cp)),
             mkop(OP_ELTWISE, 9, p=(gr.to(dev), k.to(dev), None, dx), i=(B, HW, Cp))], backend)
    assert guards_intact(obuf) and guards_intact(bbuf), "scaling layer: a write outside the tensor"
    got = out.cpu().view(B, HW, Cp)
    assert torch.equal(got[:, :, 3:], torch.zeros(B, HW, Cp - 3)), "scaling layer: a padded channel is not exactly 0"
    r1, msg = worst(f"scaling layer ({B}, {HW}, {Cp})", got, want, bound)
    assert msg is None, msg
    r2, msg = worst(f"scaling layer gradient ({B}, {HW}, {Cp})", dx.cpu().view(B, 3, HW), want_b, bound_b)
    assert msg is None, msg
    print(f"scaling layer ({B}, {HW}, {Cp}): worst err / bound {r1:.3f}; its gradient {r2:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# Part B: the plans, one launch at a time
# name -> (module switches, V, R, the conv kernel families (family, twin written) the plans must hold)
PLAN_CONFIGS = {
    "default_v1_r32": (dict(), 1, 32, {("igemm", False)}),
    "default_v2_r32": (dict(), 2, 32, {("igemm", False)}),
    "default_v3_r16": (dict(), 3, 16, {("igemm", False)}),          # a 1x1 map at tap 5: HW = 1 in the head, a 2x2 -> 1x1 pool
    "default_v1_r64": (dict(), 1, 64, {("igemm", False)}),
    "lds_v1_r64": (dict(lds_conv_min_blocks=1), 1, 64,
                   {("lds", True), ("halo", False), ("halo", True), ("halo_sm", False), ("halo_sm", True), ("igemm", False)}),
    "lds_v2_r32": (dict(lds_conv_min_blocks=1), 2, 32,
                   {("lds", True), ("halo", False), ("halo_sm", False), ("halo_sm", True), ("glds", False), ("glds", True), ("igemm", False)}),
    "no_twin_v1_r32": (dict(conv_twin=False), 1, 32, {("igemm", False)}),
    "f16_v1_r32": (dict(operand="f16"), 1, 32, {("igemm", False)}),
}


def make_module(switches, device):
    from sparsefusion_amd.lpips import LPIPS
    net = LPIPS(net='vgg')
    net.load_state_dict(lpips_ref.init_state(seed=0), strict=True)
    net = net.to(device)
    for k, v in switches.items():
        if k == "operand":
            net.set_operand(v)
        else:
            setattr(net, k, v)
    return net


def conv_family(o):
    """the kernel family run_conv (csrc/unet_ops.hip) launches for an OP_CONV record, from the record alone"""
    B, H, W, Cin, Ho, Wo, Cout, ldc, co_off, kh, kw, stride, pad, groups, tile = [o.i[k] for k in range(15)]
    if tile < 256:
        return "igemm"
    assert (tile - 256) >> 4 == 0, "a plan never carries an explicit kernel selector"
    if (o.flags & 1) or Cin % 64 or Cout % 4 or ldc % 4 or co_off % 4:
        return "lds"
    same = kh == 3 and kw == 3 and stride == 1 and pad == 1 and (Ho, Wo) == (H, W)
    if same and H == W and H in (4, 8) and not (o.flags & (2 | 16 | 128)) and 1 <= max(groups, 1) <= Cin // 64:
        return "halo_sm"
    if same and W % 16 == 0 and H % 8 == 0 and (B * Ho * Wo) % 128 == 0 and max(groups, 1) == 1 and not (o.flags & 2):
        return "halo"
    return "glds"


def conv_has_twin(o):
    return bool(o.i[14] >= 256 and max(o.i[13], 1) == 1 and o.p[5])


def op_key(o):
    """(op type, flags, conv kernel family, twin or no twin) -- what tests/test_plans_lpips_cpu.py wants covered"""
    return (o.type, o.flags, conv_family(o), conv_has_twin(o)) if o.type == OP_CONV else (o.type, o.flags, None, False)


def conv_chain(o):
    """c of derivation (c): fp32 additions on the longest accumulation chain of the kernel the op runs on"""
    K, S = o.i[3] * o.i[9] * o.i[10], max(o.i[13], 1)
    if o.i[14] < 256:
        return math.ceil(K / (128 * S)) + 32 + 8 + S
    return math.ceil(K / (32 * S)) + 32 + S


def conv_reference64(x, w, bias, prev, resid, stride, pad, relu, c):
    """x [B, H, W, Cin] and w [Cout, Cin, k, k]: float64 values of the (already rounded) operands -> want [M, Cout], bound, before ReLU |.|"""
    B = x.shape[0]
    xn = x.permute(0, 3, 1, 2)
    both = F.conv2d(torch.cat([xn, xn.abs()], 0), torch.cat([w, w.abs()], 0), None, stride=stride, padding=pad)
    Cout = w.shape[0]
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cout)      # noqa: E731
    acc, mag = rows(both[:B, :Cout]), rows(both[B:, Cout:])
    want, epi, n_epi = acc, acc.abs(), 0
    for t in (bias, resid, prev):
        if t is not None:
            want, epi, n_epi = want + t, epi + t.abs(), n_epi + 1
    bound = c * U24 * mag + n_epi * U24 * epi
    return (want.clamp(min=0) if relu else want), bound


class _Mem:
    """typed views of the plans' arenas by raw device pointer; an operand that does not lie inside an arena is a planner error"""

    def __init__(self, plans):
        self.arenas = [a.buf for p in plans for a in (p.zero, p.misc) if a.buf is not None]

    def raw(self, ptr, nbytes):
        for buf in self.arenas:
            off = ptr - buf.data_ptr()
            if 0 <= off and off + nbytes <= buf.numel():
                return buf[off:off + nbytes]
        raise AssertionError(f"an op addresses {nbytes} bytes at {ptr:#x}: outside the arenas of its plans")

    def view(self, ptr, dtype, *shape):
        n = 1
        for s in shape:
            n *= s
        return self.raw(ptr, n * torch.empty(0, dtype=dtype).element_size()).view(dtype).view(*shape)

    def host(self, ptr, dtype, *shape):
        return self.view(ptr, dtype, *shape).cpu().clone()


def _weight64(net, name, dt, cin_pad):
    """the module's fp32 conv weight behind a w-table name, rounded to the operand type: [Cout, cin_pad, 3, 3] float64.  `.T` = the
    backward-data operand W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx], restated here index by index (not by the packing code's flip)"""
    params = dict(net.named_parameters())
    if name.endswith(".T"):
        w = params[name[:-2]].detach().float().cpu()
        co, ci = w.shape[:2]
        wt = torch.empty(ci, co, 3, 3)
        for ky in range(3):
            for kx in range(3):
                wt[:, :, ky, kx] = w[:, :, 2 - ky, 2 - kx].t()
        w = wt
    else:
        w = params[name].detach().float().cpu()
    # conv1_1's three image channels are padded to 32: input channels of the forward weight, output rows of the backward-data one
    rows, cols = (32 if w.shape[0] == 3 else w.shape[0]), (32 if w.shape[1] == 3 else w.shape[1])
    out = torch.zeros(rows, cols, 3, 3)
    out[:w.shape[0], :w.shape[1]] = w
    assert cols == cin_pad, f"{name}: {cols} input channels for an op that reads {cin_pad}"
    return out.to(dt).double()


def run_plan_case(name, backend="gpu"):
    """Steps the forward and the backward plan of configuration `name` one launch at a time.  backend "gpu": sf_plan_run of one op; "ref"
    (no GPU): the float64 reference itself is written to the destination, which checks the decoding, the wiring and the conditions on the
    reference alone."""
    switches, V, R, families = PLAN_CONFIGS[name]
    dev = device_of(backend)
    net = make_module(switches, dev)
    lib = net.clib
    dt = _lib.operand_dtype(lib)
    fwd, bwd = net._plans_for(V, R, dev)
    g = torch.Generator().manual_seed(R + V)
    base = torch.rand(V, 3, R, R, generator=g)
    pred = (base + 0.15 * torch.randn(V, 3, R, R, generator=g)).clamp(0, 1)
    fwd.x_view.copy_((2 * torch.cat([pred, base], 0) - 1).reshape(2 * V, -1))
    gs = ((torch.rand(V, 1, generator=g) + 0.5) * (0.1 / V)).float()
    if net.grad_scale != 1.0:
        gs = gs * (net.grad_scale / gs.abs().max().clamp_min(1e-30))
    bwd.gscale_view.copy_(gs)
    mem = _Mem([fwd, bwd])
    params = dict(net.named_parameters())
    wname = {t.data_ptr(): n for n, t in fwd.w.items()}
    wname.update({t.data_ptr(): n for n, t in bwd.w.items()})
    vec = lambda ptr: params[wname[ptr]].detach().float().cpu().reshape(-1)      # noqa: E731  a bias / lin weight, from the module
    scaling = torch.tensor(lpips_ref.SHIFT + lpips_ref.SCALE, dtype=torch.float32)
    seen, report, failures = set(), [], []
    tap_nonzero = []

    def launch(o):
        arr = (_lib.SfOp * 1)(o)
        _lib.check(lib.sf_plan_run(arr, 1, _lib.stream_ptr()), "plan op", lib)
        torch.cuda.synchronize()

    def step(kind, k, o):
        """-> label, worst err / bound (0 for exact ops), extra text"""
        t, fl, i, p = o.type, o.flags, o.i, o.p
        dsts = []                                  # (pointer, bytes) the launch may write
        snap = [b.clone() for b in mem.arenas]

        def finish(check):
            if backend == "gpu":
                launch(o)
            res = check()
            for buf, old in zip(mem.arenas, snap):          # nothing outside the destinations changed
                base_ptr, cuts, at = buf.data_ptr(), sorted((q - buf.data_ptr(), q - buf.data_ptr() + n) for q, n in dsts
                                                            if 0 <= q - buf.data_ptr() < buf.numel()), 0
                for lo, hi in cuts + [(buf.numel(), buf.numel())]:
                    assert torch.equal(buf[at:lo], old[at:lo]), f"{kind} op {k} (type {t}): bytes outside its destination changed in [{base_ptr + at:#x}, {base_ptr + lo:#x})"
                    at = max(at, hi)
            return res

        def dst(ptr, dtype, *shape, prefill=True):
            v = mem.view(ptr, dtype, *shape)
            dsts.append((ptr, v.numel() * v.element_size()))
            if prefill:
                mem.raw(ptr, v.numel() * v.element_size()).fill_(0x7f)      # fp32 3.39e38, int16 0x7f7f: never a plausible result
            return v

        if t == OP_MEMSET:
            out = dst(p[0], torch.int32, i[0] & 0xffffffff)

            def check():
                if backend == "ref":
                    out.zero_()
                assert int(out.cpu().abs().max()) == 0, "memset: a word is not zero"
                return "memset", 0.0, f"{out.numel()} words"
            return finish(check)
        if t == OP_ELTWISE and fl == 8:
            B, HW, Cp = i[0], i[1], i[2]
            assert wname[p[1]] == "__scaling__"
            want, bound = scale_in64(mem.host(p[0], torch.float32, B, 3, HW), scaling, Cp)
            out = dst(p[3], torch.float32, B, HW, Cp)

            def check():
                if backend == "ref":
                    out.copy_(want.float())
                got = out.cpu()
                assert torch.equal(got[:, :, 3:], torch.zeros(B, HW, Cp - 3)), "scaling layer: a padded channel is not exactly 0"
                r, msg = worst("scaling layer", got, want, bound)
                assert msg is None, msg
                return "scale_in", r, ""
            return finish(check)
        if t == OP_ELTWISE and fl == 9:
            B, HW, ld = i[0], i[1], i[2]
            assert wname[p[1]] == "__scaling__"
            want, bound = scale_in_bwd64(mem.host(p[0], torch.float32, B, HW, ld), scaling)
            out = dst(p[3], torch.float32, B, 3, HW)

            def check():
                if backend == "ref":
                    out.copy_(want.float())
                r, msg = worst("scaling layer gradient", out.cpu(), want, bound)
                assert msg is None, msg
                return "scale_in_bwd", r, ""
            return finish(check)
        if t == OP_ELTWISE and fl == 7:
            n = i[0] & 0xffffffff
            dy, y = mem.host(p[0], torch.float32, n), mem.host(p[1], torch.float32, n)
            want = torch.where(y > 0, dy, torch.zeros_like(dy)).to(dt).view(torch.int16)
            out = dst(p[3], torch.int16, n)

            def check():
                if backend == "ref":
                    out.copy_(want)
                assert torch.equal(out.cpu(), want), f"relu backward: {int((out.cpu() != want).sum())} of {n} bit patterns differ"
                return "relu_bwd", 0.0, f"{n} bit patterns, {float((y > 0).double().mean()):.2f} pass"
            return finish(check)
        if t == OP_ELTWISE and fl == 4:
            n = i[0] & 0xffffffff
            a, prev = mem.host(p[0], torch.float32, n), mem.host(p[3], torch.float32, n)
            out = dst(p[3], torch.float32, n, prefill=False)
            want = prev + a                                  # one fp32 addition: exact to the bit

            def check():
                if backend == "ref":
                    out.copy_(want)
                assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)), "eltwise add: not the fp32 sum of what it read"
                return "add", 0.0, f"{n} sums"
            return finish(check)
        if t == OP_POOL:
            B, H, W, C = i[0], i[1], i[2], i[3]
            if fl == 0:
                x = mem.host(p[0], torch.float32, B, H, W, C)
                want = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
                out = dst(p[3], torch.float32, B, H // 2, W // 2, C)
            else:
                assert fl == 1
                x = mem.host(p[1], torch.float32, B, H, W, C)
                _, want = pool_expected(x, mem.host(p[0], torch.float32, B, H // 2, W // 2, C))
                out = dst(p[3], torch.float32, B, H, W, C)

            def check():
                if backend == "ref":
                    out.copy_(want)
                assert torch.equal(out.cpu(), want), f"pool flags {fl}: differs from torch at {int((out.cpu() != want).sum())} elements"
                return ("pool" if fl == 0 else "pool_bwd"), 0.0, f"({B}, {H}, {W}, {C})"
            return finish(check)
        if t == OP_LPIPS and fl == 2:
            acc = mem.host(p[2], torch.int64, i[0])
            want = (acc.double() * FIX).float()
            out = dst(p[3], torch.float32, i[0])

            def check():
                if backend == "ref":
                    out.copy_(want)
                assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)), "head sum: not the float of the fixed-point total"
                assert float(want.min()) > DIST_MIN, f"the distance {want.tolist()} is trivial"
                return "head_sum", 0.0, f"distance {want.tolist()}"
            return finish(check)
        if t == OP_LPIPS:
            Vv, HW, C = i[0], i[1], i[2]
            assert Vv == V and wname[p[1]].startswith("lin")
            feats, w = mem.host(p[0], torch.float32, 2 * Vv, HW, C), vec(p[1])
            if fl == 0:
                nz = float((feats != 0).double().mean())
                tap_nonzero.append(nz)
                assert nz >= TAP_NONZERO_MIN, f"tap {wname[p[1]]}: only {nz:.2f} of the features are non-zero"
                want, bound = head_forward64(feats, w, Vv, final=False)
                before = mem.host(p[3], torch.int64, Vv)
                out = dst(p[3], torch.int64, Vv, prefill=False)

                def check():
                    if backend == "ref":
                        out.copy_(before + torch.round(want / FIX).long())
                    r, msg = worst(f"head forward {wname[p[1]]}", (out.cpu() - before).double() * FIX, want, bound)
                    assert msg is None, msg
                    return "head_fwd", r, f"({Vv}, {HW}, {C}) non-zero {nz:.2f}"
                return finish(check)
            assert fl == 1
            want, bound = head_backward64(feats, w, Vv, mem.host(p[2], torch.float32, Vv))
            out = dst(p[3], torch.float32, Vv, HW, C)

            def check():
                if backend == "ref":
                    out.copy_(want.float())
                r, msg = worst(f"head backward {wname[p[1]]}", out.cpu(), want, bound)
                assert msg is None, msg
                return "head_bwd", r, f"({Vv}, {HW}, {C})"
            return finish(check)
        assert t == OP_CONV, f"an op type {t} the LPIPS plans are not known to hold"
        B, H, W, Cin, Ho, Wo, Cout, ldc, co_off, kh, kw, stride, pad, groups, tile = [i[j] for j in range(15)]
        assert not (fl & ~(1 | 4 | 32)) and kh == 3 and kw == 3 and ldc == Cout and co_off == 0, "a conv form this test does not restate"
        fam, twin = conv_family(o), conv_has_twin(o)
        seen.add((fam, twin))
        M = B * Ho * Wo
        x = mem.host(p[0], torch.float32 if fl & 1 else dt, B, H, W, Cin).float().to(dt).double()      # exact when the source is a 16-bit twin
        w64 = _weight64(net, wname[p[1]], dt, Cin)
        assert w64.shape == (Cout, Cin, 3, 3), f"{wname[p[1]]}: weight shape {tuple(w64.shape)} for a {Cin} -> {Cout} conv"
        bias = vec(p[2]).double() if p[2] else None
        resid = mem.host(p[4], torch.float32, M, Cout).double() if p[4] else None
        prev = mem.host(p[3], torch.float32, M, Cout).double() if fl & 4 else None
        want, bound = conv_reference64(x, w64, bias, prev, resid, stride, pad, bool(fl & 32), conv_chain(o))
        rms = float(want.pow(2).mean().sqrt())
        tight = float(bound.median()) / max(rms, 1e-300)
        assert tight <= BOUND_MEDIAN_MAX, f"{kind} op {k} {wname[p[1]]}: median bound / rms = {tight:.2e}: the bound is too loose to see an error"
        out = dst(p[3], torch.float32, M, Cout, prefill=not (fl & 4))
        tw = dst(p[5], torch.int16, M, Cout) if twin else None
        if max(groups, 1) > 1:
            dsts.append((p[5], max(groups, 1) * M * ((Cout + 15) // 16 * 16) * 4))      # the split-K workspace

        def check():
            if backend == "ref":
                out.copy_(want.float())
                if tw is not None:
                    tw.copy_(want.float().to(dt).view(torch.int16))
            got = out.cpu()
            r, msg = worst(f"{kind} op {k} conv {wname[p[1]]} ({fam}, tile {tile}, groups {groups})", got, want, bound)
            assert msg is None, msg
            if tw is not None:        # the twin is the operand-type rounding of the fp32 value the launch stored, bit for bit
                assert torch.equal(tw.cpu(), got.to(dt).view(torch.int16)), f"{kind} op {k} conv {wname[p[1]]}: the twin is not the rounding of the stored fp32 value"
            return f"conv {fam}{'+twin' if twin else ''}", r, f"{wname[p[1]]} ({B}, {H}, {Cin}->{Cout}) tile {tile} groups {groups} c {conv_chain(o)} median bound / rms {tight:.1e}"
        return finish(check)

    keys = set()
    for kind, plan in (("fwd", fwd), ("bwd", bwd)):
        for k, o in enumerate(plan.ops):
            keys.add(op_key(o))
            try:
                label, r, text = step(kind, k, o)
            except AssertionError as e:          # every launch is judged, the report names them all
                failures.append(f"{kind} op {k}: {e}")
                label, r, text = "FAILED", float("inf"), str(e)[:120]
            report.append(f"{name} {kind} op {k:2d} {label:18s} err / bound {r:.3f}  {text}")
    print("\n".join(report))
    assert not failures, f"{len(failures)} launches of {name} outside their expectation:\n" + "\n".join(failures)
    check_wiring(fwd, bwd, wname, V)
    # the last op of each plan wrote what the module reads
    last_f, last_b = fwd.ops[-1], bwd.ops[-1]
    assert torch.equal(fwd.dist_view.cpu().view(torch.int32).flatten(), mem.host(last_f.p[3], torch.int32, V))
    assert torch.equal(bwd.out_view.cpu().view(torch.int32).flatten(), mem.host(last_b.p[3], torch.int32, V * 3 * R * R))
    assert seen == families, f"{name}: conv kernel families {sorted(seen)}, expected {sorted(families)}"
    assert len(tap_nonzero) == 5
    return keys


def check_wiring(fwd, bwd, wname, V):
    """The dataflow of the two plans, from the op records alone: which buffer every op of the backward must read is fixed by which forward
    op wrote it.  (A per-launch comparison cannot see an op that reads the WRONG buffer consistently, e.g. sample V + s instead of s.)"""
    conv_out, conv_in, head_feats_of, pool_of = {}, {}, {}, {}
    producer = {}                                   # destination pointer -> forward op that wrote it last
    for o in fwd.ops:
        if o.type == OP_CONV:
            conv_out[wname[o.p[1]]], conv_in[wname[o.p[1]]] = o.p[3], (o.p[0], o.i[0], o.i[1], o.i[3])
            producer[o.p[3]] = o
            if conv_has_twin(o):
                producer[o.p[5]] = o
        elif o.type == OP_POOL:
            pool_of[o.p[3]] = o
            producer[o.p[3]] = o
        elif o.type == OP_LPIPS and o.flags == 0:
            head_feats_of[wname[o.p[1]]] = (o.p[0], o.i[1], o.i[2])
            assert o.i[0] == V and o.p[0] in producer and producer[o.p[0]].type == OP_CONV, "a head reads something no conv wrote"
        elif o.type == OP_ELTWISE and o.flags == 8:
            producer[o.p[3]] = o
    for o in fwd.ops:                               # every forward conv reads the fp32 output (or the twin) of the op before it in the chain
        if o.type == OP_CONV:
            assert o.p[0] in producer, f"forward conv {wname[o.p[1]]} reads a buffer no forward op wrote"
            assert o.i[0] == 2 * V
    grad_of = {}                                    # forward tensor pointer -> the backward buffer that holds its gradient
    ops = bwd.ops
    for k, o in enumerate(ops):
        if o.type == OP_LPIPS:
            assert o.flags == 1 and o.i[0] == V
            assert (o.p[0], o.i[1], o.i[2]) == head_feats_of[wname[o.p[1]]], f"head gradient {wname[o.p[1]]} reads another tensor than its forward head"
            grad_of[o.p[0]] = o.p[3]
        elif o.type == OP_CONV:
            name = wname[o.p[1]]
            assert name.endswith(".T"), "a backward conv on a forward weight"
            relu = ops[k - 1]
            assert relu.type == OP_ELTWISE and relu.flags == 7 and relu.p[3] == o.p[0], "a backward conv does not read the ReLU mask op before it"
            y = conv_out[name[:-2]]
            assert relu.p[1] == y, f"{name}: the ReLU mask is taken from another tensor than the forward output of that layer (sample 0 first)"
            assert relu.p[0] == grad_of[y], f"{name}: the ReLU backward reads another gradient than that of its layer's output"
            assert o.i[0] == V and relu.i[0] == V * o.i[1] * o.i[2] * o.i[3]
            src = conv_in[name[:-2]]
            assert (o.i[1], o.i[6]) == (src[2], src[3]), f"{name}: gradient shape differs from the forward input"
            fsrc = producer[src[0]]                  # the forward op whose output (or twin) the layer read
            grad_of[fsrc.p[3]] = o.p[3]
        elif o.type == OP_POOL:
            assert o.flags == 1 and o.i[0] == V
            f = pool_of.get(next(ptr for ptr, g in grad_of.items() if g == o.p[0]))
            assert f is not None and f.p[0] == o.p[1] and (f.i[1], f.i[2], f.i[3]) == (o.i[1], o.i[2], o.i[3]), "pool backward: not the forward pool's input"
            add = ops[k + 1]
            assert add.type == OP_ELTWISE and add.flags == 4 and add.p[0] == o.p[3] and add.p[3] == grad_of[f.p[0]], \
                "the routed pool gradient is not added to the head gradient of the tap it came from"
        elif o.type == OP_ELTWISE and o.flags == 9:
            first = next(f for f in fwd.ops if f.type == OP_ELTWISE and f.flags == 8)
            assert o.p[0] == grad_of[first.p[3]] and o.i[0] == V, "the image gradient is not taken from the gradient of the scaled input"

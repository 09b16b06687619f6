"""Every launch of the SD-VAE plans (sparsefusion_amd/vae.py::_VaePlan), stepped one op at a time (run_plan_case) in the pattern of
tests/lpips_cases.py Part B: the operands and destinations of an op are decoded from its record alone, what it reads is copied to the
host, every destination is prefilled with the 0x7f pattern (accumulate and in-place forms excepted), the op is launched alone, and every
destination element is compared with the float64 evaluation of that op ON THE VALUES IT ACTUALLY READ -- no error is carried from one
launch to the next, so each bound is that of a single launch.  After each launch every byte of both arenas of both plans outside the op's
destinations must be unchanged; a destination is a strided region where ldc != Cout or co_off != 0 (the 24 / 28 pad lanes of the 32-wide
moment / latent rows are "outside" and must stay exactly 0), and a split-K workspace is a destination.

What each op is held to.  No constant is fitted to a kernel's output; the margins of the first recorded run are in
profiles/vae_op_parity_margins.log.
  OP_MEMSET: every word zero.  ELTWISE 2 / 3 (pack in, unpack out): torch.equal with the permutation, pad channels exactly 0.
  ELTWISE 5 (device pack of a B operand): the packed buffer, unpacked with hostemu.plan_interp.unpack_weights, is the operand-type rounding
    of the source bit for bit, pad rows and columns 0; both orientations.
  ELTWISE 6: norm_cases.softmax_ref64, derivation (c) of norm_cases.py, through check_bf16 with its cap MISMATCH_MAX.
  OP_GN_FINALIZE: a double sum of `tiles` partials in some order: tiles 2^-53 sum|partial| (the reference sum is exact: math.fsum).
  OP_GN_ACT: norm_cases.gn_act_ref64, derivation (a), with the addition counts of the kernel gn_geometry names.  With flag 2 the reference
    is evaluated on the statistics buffer the launch read (they add nothing to the bound), and that buffer is checked separately against the
    float64 sums of the fp32 tensor the GroupNorm reads under READY_COUNTS -- which ties the partials of a conv epilogue to the values the
    same conv stored.  k_gn_stats(_px) ADD into the statistics buffer: the increment is checked; k_gn_one must leave it alone.
  OP_CONV: derivation (c) of lpips_cases.py, c = conv_chain(o), on the float64 conv of the operand-rounded activations and weights.  The
    forms are restated here index by index, not through the kernel's address code: output (oy, ox), tap (ky, kx) reads input
    (oy stride + ky - pad, ox stride + kx - pad) where that lies inside [0, H) x [0, W) and 0 elsewhere (so a stride-2 conv with pad 0 and
    an explicit output size H / 2 pads right and bottom only); with flag 16 input (y, x) is element (y >> 1, x >> 1) of the stored half-size
    map; an fp32 A operand is rounded to the operand type as the kernel does on load (nothing added to the bound); residual, accumulate
    (flag 4) and bias are the epilogue additions; the result goes to columns co_off .. co_off + Cout of rows of ldc floats.  A named layer's
    weight is the MODULE's parameter rounded to the operand type (a packing error shows); a per-sample GEMM's weight is what the packed
    buffer holds.  A twin is the rounding of the stored fp32 value bit for bit; the [tile][group][2] partials of flag 128 are the float64
    sums of the stored output per 128-pixel tile under READY_COUNTS.
End to end: the output of the stepped run is bit-equal to a plain encode / decode of the same input (backend "gpu"); with backend "ref"
(no GPU: the float64 reference is written to the destinations) it is within the whole-model tolerance of tests/test_gpu_vae.py of
oracle/vae_ref.py, which shows that the references restate the model.
check_wiring: the dataflow from the op records alone, which a per-launch check cannot see.

Nothing in the arena, guard or stepping code is specific to the VAE: an op is decoded by (type, flags) in _DECODERS, so the UNet and EFT
plans can follow by adding decoders."""
import contextlib
import io
import math

import torch

import lpips_cases as lc
import norm_cases as nc
from hostemu.plan_interp import unpack_weights
from lpips_cases import BOUND_MEDIAN_MAX, OP_CONV, OP_ELTWISE, OP_MEMSET, U24, conv_chain, conv_family, conv_has_twin, device_of, worst
from norm_cases import OP_GN_ACT, OP_GN_FINALIZE, READY_COUNTS
from oracle import vae_ref
from sparsefusion_amd import _lib

REL_MODEL = 2e-2                  # tests/test_gpu_vae.py: relative L2 of a whole encode / decode (backend "ref" only)
ATTN_PEAK_MIN = 2.0               # median over rows of max_j p_j * HW: the attention of the test state is not uniform
S = vae_ref.SMALL


# ---------------------------------------------------------------------------------------------------------------------------------
# the kind of a launch, and the configurations
def launch_kind(o):
    """conv: (flags, kernel family, twin written, k, stride, channel-tile width of an LDS-tiled launch, split-K, ldc != Cout);
    GroupNorm: (flags, kernel, NT, NCH, channels per group); everything else: (type, flags)"""
    i = o.i
    if o.type == OP_CONV:
        return ("conv", o.flags, conv_family(o), conv_has_twin(o), i[9], i[11], (i[14] & 15) if i[14] >= 256 else 0, max(i[13], 1) > 1, i[7] != i[6])
    if o.type == OP_GN_ACT:
        G = i[8] or 8
        geo = nc.gn_geometry(i[0], i[1], i[2], i[3], G, o.flags)
        return ("gn", o.flags, geo["kernel"], geo.get("NT"), geo.get("NCH"), (i[2] + i[3]) // G)
    return (o.type, o.flags)


_C256 = dict(S, ch=256, ch_mult=(1, 1), resolution=64)
# name -> (configuration, module switches, B, kinds of launch the configuration is there for: tests/test_plans_vae_cpu.py (ii))
CONFIGS = {
    # the implicit-GEMM forms: fp32 and twin-less A, the 32-wide rows, the statistics passes k_gn_stats_px; the per-sample attention
    "small_b1": (S, dict(), 1, {("conv", 1, "igemm", False, 3, 1, 0, False, False), ("conv", 1, "igemm", False, 1, 1, 0, False, True),
                                ("conv", 0, "igemm", False, 3, 1, 0, False, False), ("conv", 1, "igemm", False, 1, 1, 0, False, False),
                                ("conv", 0, "igemm", False, 3, 1, 0, True, True), ("conv", 1, "igemm", False, 3, 2, 0, False, False),
                                ("conv", 4, "igemm", False, 3, 1, 0, False, False), ("conv", 17, "igemm", False, 3, 1, 0, False, False),
                                ("gn", 0, "k_gn_stats_px", None, None, 4), ("gn", 1, "k_gn_stats_px", None, None, 8),
                                (OP_MEMSET, 0), (OP_ELTWISE, 2), (OP_ELTWISE, 3), (OP_ELTWISE, 5), (OP_ELTWISE, 6)}),
    # an odd batch: k_gn_one by its second rule (B * 32 >= 64 workgroups, <= 2^19 elements), the Upsample on k_conv_lds with an fp32 A operand
    "small_b3": (S, dict(), 3, {("conv", 0, "igemm", False, 1, 1, 0, False, False), ("conv", 145, "lds", True, 3, 1, 4, False, False),
                                ("gn", 0, "k_gn_one", 256, 4, 4), ("gn", 1, "k_gn_one", 256, 2, 8)}),
    # B * 32 = 256 workgroups: k_gn_one on GroupNorm(32) with 4 and 8 channels per group by its first rule (third item)
    "small_b8": (S, dict(), 8, {("gn", 0, "k_gn_one", 256, 2, 4), ("gn", 0, "k_gn_one", 256, 2, 8), ("conv", 0, "igemm", False, 3, 1, 0, False, True)}),
    # the LDS-tiled kernels at the smallest size: epilogue partials -> OP_GN_FINALIZE -> flag 2, twins, the nearest-x2 view on k_conv3_halo
    "small_lds_b1": (S, dict(lds_conv_min_blocks=1), 1, {("conv", 128, "halo", False, 3, 1, 4, False, False), ("conv", 132, "halo", False, 3, 1, 4, False, False),
                                                         ("conv", 129, "lds", False, 3, 1, 4, False, False), ("conv", 129, "lds", False, 1, 1, 4, False, False),
                                                         ("gn", 2, "ready", None, None, 4), ("gn", 2, "ready", None, None, 8), ("gn", 3, "ready", None, None, 8),
                                                         (OP_GN_FINALIZE, 0)}),
    # the canonical widths 256 -> 512 at B = 4: both channel-tile widths of k_conv3_halo, k_conv_glds 1x1 and stride 2 with twins
    "m24_r64_b4": (dict(S, ch_mult=(2, 4), resolution=64), dict(), 4,
                   {("conv", 0, "glds", False, 1, 1, 4, False, False), ("conv", 0, "glds", False, 1, 1, 8, False, False),
                    ("conv", 0, "halo", True, 3, 1, 4, False, False), ("conv", 1, "lds", False, 1, 1, 4, False, False),
                    ("conv", 128, "glds", True, 3, 2, 4, False, False), ("conv", 128, "halo", False, 3, 1, 8, False, False),
                    ("conv", 132, "halo", False, 3, 1, 8, False, False), ("conv", 144, "halo", True, 3, 1, 8, False, False),
                    ("gn", 2, "ready", None, None, 16), ("gn", 3, "ready", None, None, 16)}),
    # levels of equal width (no twin behind the Down / Upsample output), 256 -> 256 at M = 16384: the 128-channel tile
    "c256_r64_b4": (_C256, dict(), 4, {("conv", 0, "halo", True, 3, 1, 8, False, False), ("conv", 128, "glds", False, 3, 2, 4, False, False),
                                       ("conv", 129, "lds", False, 3, 1, 8, False, False), ("conv", 144, "halo", False, 3, 1, 8, False, False)}),
    "c256_r64_b2": (_C256, dict(), 2, {("conv", 144, "halo", False, 3, 1, 4, False, False)}),
    # 512 channels on small maps: split-K on the implicit-GEMM tail (3x3, stride 2, the 8-of-32 row), 16 channels per group on the statistics pass
    "m44_r32_b1": (dict(S, ch_mult=(4, 4)), dict(), 1, {("conv", 0, "igemm", False, 3, 1, 0, True, True), ("conv", 0, "igemm", False, 3, 2, 0, True, False),
                                                        ("conv", 1, "igemm", False, 3, 1, 0, False, False), ("gn", 0, "k_gn_stats_px", None, None, 16)}),
}
CANONICAL_BATCHES = (1, 2, 8)
# Kinds of the canonical plans that no configuration above holds: each needs >= 256 workgroup tiles of 128 channels on 512-channel maps
# (M >= 8192 rows of 512 -> 512 3x3: >= 150 GFLOP of float64 reference per conv).  canonical kind -> (the stepped kind that differs from it in
# the channel-tile width alone, the per-op test that runs that instantiation: the kind itself at M = 256, run_exception_case below)
EXCEPTIONS = {
    ("conv", 128, "glds", False, 3, 2, 8, False, False): (("conv", 128, "glds", False, 3, 2, 4, False, False),
                                                          "test_gpu_vae_ops.py::test_exception_kinds_on_the_128_channel_tile (k_conv_glds<8, 4, true>, stride 2)"),
    ("conv", 128, "glds", True, 3, 2, 8, False, False): (("conv", 128, "glds", True, 3, 2, 4, False, False),
                                                         "test_gpu_vae_ops.py::test_exception_kinds_on_the_128_channel_tile (k_conv_glds<8, 4, true>, stride 2)"),
    ("conv", 129, "lds", False, 1, 1, 8, False, False): (("conv", 129, "lds", False, 1, 1, 4, False, False),
                                                         "test_gpu_vae_ops.py::test_exception_kinds_on_the_128_channel_tile (k_conv_lds_gn<8, true>, 1x1)"),
}


def make_module(cfg, switches, device):
    from sparsefusion_amd.vae import AutoencoderKL
    net = AutoencoderKL(ddconfig={k: v for k, v in cfg.items() if k != "embed_dim"}, embed_dim=cfg["embed_dim"])
    net.load_state_dict(vae_ref.init_state(vae_ref.vae_param_spec(cfg), seed=0), strict=True)
    net = net.to(device)
    for k, v in switches.items():
        setattr(net, k, v)
    return net


def sizing_plans(cfg, switches, B):
    """both plans in sizing mode (fake device pointers, no arena): the op records are those of the real plans"""
    from sparsefusion_amd.vae import _VaePlan
    net = make_module(cfg, switches, "cpu")
    return [_VaePlan(net, kind, B, "cpu").build() for kind in ("enc", "dec")]


def inputs(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    R = cfg["resolution"]
    f = 2 ** (len(cfg["ch_mult"]) - 1)
    return torch.rand(B, cfg["in_channels"], R, R, generator=g) * 2 - 1, torch.randn(B, cfg["z_channels"], R // f, R // f, generator=g)


# ---------------------------------------------------------------------------------------------------------------------------------
# references
def conv_input64(xs, H, W, Ho, Wo, k, stride, pad, ups):
    """xs: the stored input [B, Hs, Ws, Cin] (float64 of the rounded operand) -> [B, (Ho - 1) stride + k, (Wo - 1) stride + k, Cin]: the
    array a VALID conv of that stride reads, built from the rule of the header comment index by index"""
    B, Cin = xs.shape[0], xs.shape[3]
    if ups:
        assert (xs.shape[1], xs.shape[2]) == (H // 2, W // 2) and H % 2 == 0 and W % 2 == 0
        xs = xs[:, torch.arange(H) // 2][:, :, torch.arange(W) // 2]
    assert xs.shape[1:3] == (H, W)
    nh, nw = (Ho - 1) * stride + k, (Wo - 1) * stride + k
    xp = torch.zeros(B, nh, nw, Cin, dtype=torch.float64)
    ys, xcols = torch.arange(nh) - pad, torch.arange(nw) - pad          # padded row r holds input row r - pad
    yin, xin = (ys >= 0) & (ys < H), (xcols >= 0) & (xcols < W)
    rows, cols = torch.nonzero(yin).flatten(), torch.nonzero(xin).flatten()
    xp[:, rows[:, None], cols[None, :]] = xs[:, ys[rows][:, None], xcols[cols][None, :]]
    return xp


def conv_reference64(xp, w, bias, prev, resid, stride, c, dev="cpu"):
    """lpips_cases.conv_reference64 for an explicit input array (conv_input64) -> want [M, Cout], bound: the same expression, written as
    one float64 matrix product per tap -- output (oy, ox), tap (ky, kx) reads xp[oy stride + ky, ox stride + kx] -- so that the products
    can run where float64 is fast (dev: the GPU when there is one: torch's own matmul, none of this project's kernels)."""
    B, nh, nw, Cin = xp.shape
    Cout, k = w.shape[0], w.shape[2]
    Ho, Wo = (nh - k) // stride + 1, (nw - k) // stride + 1
    xd, wd = xp.to(dev), w.to(dev)
    acc = torch.zeros(B * Ho * Wo, Cout, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(acc)
    for ky in range(k):
        for kx in range(k):
            a = xd[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :].reshape(B * Ho * Wo, Cin)
            wt = wd[:, :, ky, kx].t()
            acc += a @ wt
            mag += a.abs() @ wt.abs()
    acc, mag = acc.cpu(), mag.cpu()
    want, epi, n_epi = acc, acc.abs(), 0
    for t in (bias, resid, prev):
        if t is not None:
            want, epi, n_epi = want + t, epi + t.abs(), n_epi + 1
    return want, c * U24 * mag + n_epi * U24 * epi


def tile_sums64(v, cg, fam, B, Ho, Wo):
    """v [M, C] float64 -> the (sum, sum of squares) per (128-pixel tile, group of cg channels) [M / 128, C / cg, 2] and their bound
    under READY_COUNTS (norm_cases.py (a): an fp32 chain of at most 32 values per thread, doubles above).  The 128 pixels of a tile are
    consecutive rows of the [M, C] matrix on k_conv_lds / k_conv_glds and an 8 x 16 block of the map on k_conv3_halo (csrc/conv_halo.h:
    blocks of an image in row-major order, image after image) -- OP_GN_FINALIZE adds the tiles of an image up either way."""
    M, C = v.shape
    if fam == "halo":
        assert Ho % 8 == 0 and Wo % 16 == 0
        t = v.view(B, Ho // 8, 8, Wo // 16, 16, C // cg, cg).permute(0, 1, 3, 2, 4, 5, 6).reshape(M // 128, 128, C // cg, cg)
    else:
        t = v.view(M // 128, 128, C // cg, cg)
    s, q, sa = t.sum((1, 3)), (t * t).sum((1, 3)), t.abs().sum((1, 3))
    return torch.stack([s, q], -1), torch.stack([READY_COUNTS[0] * U24 * sa, READY_COUNTS[1] * U24 * q], -1)


def _stats_ratio(tag, got, sums, sums_bound):
    """norm_cases.check_stats, its printed margin line reduced to the figure (it goes into the launch's own line)"""
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        nc.check_stats(tag, got, sums, sums_bound)
    return buf.getvalue().strip().rsplit(" ", 1)[-1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the stepper
class _Step:
    """One launch: typed views of what it reads (host copies) and writes (destinations, device views), the arena guard."""

    def __init__(self, mem, backend):
        self.mem, self.backend = mem, backend
        self.snap = [b.clone() for b in mem.arenas]
        self.dsts = []                             # (pointer of the first element, rows, bytes per row, row pitch in bytes)

    def host(self, ptr, dtype, *shape):
        return self.mem.host(ptr, dtype, *shape)

    def dst(self, ptr, dtype, rows, cols, ld=None, off=0, prefill=True):
        """columns off .. off + cols of `rows` rows of ld elements at ptr -> the (strided) device view"""
        ld = cols if ld is None else ld
        es = torch.empty(0, dtype=dtype).element_size()
        whole = self.mem.raw(ptr, rows * ld * es)
        self.dsts.append((ptr + off * es, rows, cols * es, ld * es))
        if prefill:
            whole.view(rows, ld * es)[:, off * es:(off + cols) * es].fill_(0x7f)      # fp32 3.39e38, bf16 3.39e38, f64 1.4e306: never a plausible result
        return whole.view(dtype).view(rows, ld)[:, off:off + cols]

    def outside_unchanged(self):
        for buf, old in zip(self.mem.arenas, self.snap):
            if torch.equal(buf, old):
                continue
            changed = buf != old
            base = buf.data_ptr()
            for ptr, rows, nbytes, pitch in self.dsts:
                if 0 <= ptr - base < buf.numel():
                    torch.as_strided(changed, (rows, nbytes), (pitch, 1), ptr - base).fill_(False)
            if bool(changed.any()):
                at = int(changed.nonzero()[0])
                raise AssertionError(f"{int(changed.sum())} bytes outside the destinations changed, the first at arena offset {at} ({base + at:#x}): {int(old[at])} -> {int(buf[at])}")


def step_op(mem, backend, o, cx):
    """One op, alone: decode, copy what it reads, prefill, launch (backend "gpu") or write the reference (backend "ref"), compare, guard.
    cx: tag, dt (operand type), wname (device pointer -> parameter name), params (name -> fp32 tensor on the host), attn_peaks (a list)
    -> (label, worst err / bound, text); raises AssertionError with everything that failed"""
    st = _Step(mem, backend)
    cx = dict(cx, vec=lambda ptr: cx["params"][cx["wname"][ptr]].reshape(-1))      # a bias / GroupNorm weight, from the module
    key = (o.type, o.flags) if (o.type, o.flags) in _DECODERS else (o.type, None)
    assert key in _DECODERS, f"an op (type {o.type}, flags {o.flags}) this stepper does not restate"
    ref_write, check = _DECODERS[key](st, o, cx)
    if backend == "gpu":
        lib = _lib.lib()
        _lib.check(lib.sf_plan_run((_lib.SfOp * 1)(o), 1, _lib.stream_ptr()), "plan op", lib)
        torch.cuda.synchronize()
    elif backend == "emu" and o.type == OP_CONV and o.i[14] >= 256 and max(o.i[13], 1) == 1:
        emu_conv(o)
    else:
        ref_write()
    errs, res = [], None
    for f in (check, st.outside_unchanged):
        try:
            res = f() or res
        except AssertionError as e:
            errs.append(str(e))
    if errs:
        raise AssertionError("; ".join(errs))
    return res


def emu_conv(o):
    """an LDS-tiled conv launch on CPU fibers: the kernel source itself (tests/hostemu/conv_lds_emu.cpp), on host memory"""
    import ctypes as C
    from test_hostemu_conv_lds import _lib as emu_lib
    i, p, fl = o.i, o.p, o.flags
    ring = {"lds": 0, "glds": 4, "halo": 7}[conv_family(o)]          # run_conv's defaults: ring depth 4
    stats = torch.zeros(i[0] * (i[6] // max(i[15], 1)) * 2, dtype=torch.float64)      # (the emulator finalises the partials too; not looked at)
    ptr = lambda v: C.c_void_p(v or 0)          # noqa: E731
    rc = emu_lib().emu_conv_lds(ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(p[3]), ptr(p[4]), *[i[j] for j in range(9)], i[9], i[11], i[12], i[14] & 15,
                                fl & 1, 1 if fl & 4 else 0, 1 if fl & 16 else 0, 0, ptr(p[6] if fl & 128 else 0), i[15] if fl & 128 else 0,
                                ptr(stats.data_ptr()), ring, ptr(p[5] if conv_has_twin(o) else 0))
    assert rc == 0, f"the emulator refused the conv ({rc})"


def run_plan_case(name, backend="gpu"):
    """Steps the encode and the decode plan of configuration `name` one launch at a time.  backend "gpu": sf_plan_run of one op; "ref" (no
    GPU): the float64 reference itself is written to the destination, which checks the decoding, the wiring and the conditions on the
    reference alone; "emu" (no GPU): as "ref", but the LDS-tiled convs run the kernel source on CPU fibers (tests/hostemu).  Prints one margin line per launch; a failing case reports every failing launch.  -> the kinds of launch stepped"""
    cfg, switches, B, listed = CONFIGS[name]
    dev = torch.device(device_of(backend))
    net = make_module(cfg, switches, dev)
    lib = _lib.lib()
    dt = _lib.operand_dtype(lib)
    assert dt == torch.bfloat16, "the f16 operand build is not stepped (unpack_weights reads bf16)"
    plans = {kind: net._plan(kind, B, dev) for kind in ("enc", "dec")}
    img, z = inputs(cfg, B, seed=11 + B)
    plans["enc"].x_view.copy_(img.reshape(B, -1))
    plans["dec"].x_view.copy_(z.reshape(B, -1))
    mem = lc._Mem(list(plans.values()))
    params = {n: t.detach().float().cpu() for n, t in net.named_parameters()}
    report, failures, kinds, attn_peaks = [], [], set(), []

    for kind, plan in plans.items():
        wname = {t.data_ptr(): n for n, t in plan.w.items()}
        for k, o in enumerate(plan.ops):
            kinds.add(launch_kind(o))
            tag = f"{name} {kind} op {k:3d}"
            try:
                label, r, text = step_op(mem, backend, o, dict(tag=tag, dt=dt, wname=wname, params=params, attn_peaks=attn_peaks))
            except AssertionError as e:          # every launch is judged, the report names them all
                failures.append(f"{tag} kind {launch_kind(o)}: {e}")
                label, r, text = "FAILED", float("inf"), str(e)[:160]
            report.append(f"margin {tag} {label:22s} err / bound {r:.3f}  {text}")
        check_wiring(plan, wname)
    print("\n".join(report))
    assert not failures, f"{len(failures)} launches of {name} outside their expectation:\n" + "\n".join(failures)
    assert listed <= kinds, f"{name} does not hold the kinds it is listed for: {sorted(listed - kinds, key=str)}"
    assert attn_peaks and min(attn_peaks) >= ATTN_PEAK_MIN, f"degenerate attention: median row peak * HW {attn_peaks}"
    # end to end: the stepped run is the run the product does
    for kind, x in (("enc", img), ("dec", z)):
        stepped = plans[kind].out_view.clone().view(B, *plans[kind].out_shape).cpu()
        assert bool(torch.isfinite(stepped).all())
        if backend == "gpu":
            plain = (net.encode(x.to(dev)).parameters if kind == "enc" else net.decode(x.to(dev))).cpu()
            assert torch.equal(plain.view(torch.int32), stepped.view(torch.int32)), \
                f"{name} {kind}: the stepped run differs from a plain run at {int((plain != stepped).sum())} of {plain.numel()} elements"
        else:
            sd = {n: t for n, t in params.items()}
            with torch.no_grad():
                want = vae_ref.encode_moments(sd, cfg, x) if kind == "enc" else vae_ref.decode(sd, cfg, x)
            rel = float((stepped - want).norm() / want.norm())
            print(f"{name} {kind}: the chained references against oracle/vae_ref.py: rel-L2 {rel:.2e}")
            assert rel < REL_MODEL, f"{name} {kind}: the chained float64 references are {rel:.3g} off the oracle: they do not restate the model"
    return kinds


# ---------------------------------------------------------------------------------------------------------------------------------
# decoders: (step, op, context) -> (what backend "ref" writes, the check -> (label, worst err / bound, text))
def _dec_memset(st, o, cx):
    out = st.dst(o.p[0], torch.int32, 1, o.i[0] & 0xffffffff)

    def check():
        assert int(out.cpu().abs().max()) == 0, "memset: a word is not zero"
        return "memset", 0.0, f"{out.numel()} words"
    return out.zero_, check


def _dec_pack_in(st, o, cx):
    B, HW, Cc, Cx, Cp = [o.i[k] for k in range(5)]
    assert Cc == 0 and not o.p[0], "pack in: a conditioning source the VAE plans do not have"
    x = st.host(o.p[1], torch.float32, B, Cx, HW)
    want = torch.zeros(B, HW, Cp)
    want[:, :, :Cx] = x.permute(0, 2, 1)
    out = st.dst(o.p[3], torch.float32, B * HW, Cp)

    def check():
        got = out.cpu().view(B, HW, Cp)
        assert torch.equal(got[:, :, Cx:].view(torch.int32), torch.zeros(B, HW, Cp - Cx, dtype=torch.int32)), "pack in: a pad channel is not exactly 0"
        assert torch.equal(got, want), f"pack in: {int((got != want).sum())} elements differ from the permutation"
        return "pack_in", 0.0, f"({B}, {Cx}, {HW}) -> rows of {Cp}"
    return (lambda: out.copy_(want.view(B * HW, Cp))), check


def _dec_unpack_out(st, o, cx):
    B, HW, C, ldi = [o.i[k] for k in range(4)]
    want = st.host(o.p[0], torch.float32, B, HW, ldi)[:, :, :C].permute(0, 2, 1).contiguous().view(B, C * HW)
    out = st.dst(o.p[3], torch.float32, B, C * HW)

    def check():
        assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)), "unpack out: differs from the permutation"
        return "unpack_out", 0.0, f"rows of {ldi} -> ({B}, {C}, {HW})"
    return (lambda: out.copy_(want)), check


def _dec_pack_act(st, o, cx):
    N, K, ld, T = [o.i[k] for k in range(4)]
    assert T in (0, 1)
    src = st.host(o.p[0], torch.float32, K if T else N, ld)
    nfr, kch = (N + 15) // 16, (K + 31) // 32
    want = torch.zeros(nfr * 16, kch * 32)
    want[:N, :K] = src[:K, :N].t() if T else src[:N, :K]          # W[n][c] = src[c * ld + n] (T = 1) or src[n * ld + c]
    want = want.to(cx["dt"])
    out = st.dst(o.p[3], torch.int16, 1, nfr * kch * 512)

    def ref_write():
        packed, _ = nc.pack_conv(want.float()[:N, :K].reshape(N, K, 1, 1).contiguous(), "cpu")      # the host packer stands in for the launch
        out.copy_(packed.view(1, -1))

    def check():
        buf = out.cpu().contiguous()
        got = unpack_weights(buf.data_ptr(), nfr * 16, kch * 32, 1)[:, 0, :].to(cx["dt"])
        diff = got.view(torch.int16) != want.view(torch.int16)
        assert not bool(diff.any()), f"pack (T = {T}): {int(diff.sum())} of {diff.numel()} unpacked elements are not the rounding of the source (pad rows / columns included)"
        return f"pack_act T={T}", 0.0, f"N {N} K {K} ld {ld}"
    return ref_write, check


def _dec_softmax(st, o, cx):
    R, N, scale = o.i[0], o.i[1], o.f[0]
    x = st.host(o.p[0], torch.float32, R, N)
    want, delta = nc.softmax_ref64(x, scale)
    peak = float((want.max(1).values * N).median())
    cx["attn_peaks"].append(peak)
    out = st.dst(o.p[3], torch.int16, R, N)

    def check():
        fig = nc.check_bf16(f"{cx['tag']} softmax rows", out.cpu().view(cx["dt"]), want, delta, log=False)
        return "softmax_rows", fig["worst"], f"({R}, {N}) worst (err - half_ulp)/delta {fig['used']:.3f} mismatch {fig['mismatch']:.2e} median delta/half_ulp {fig['median']:.2e} median row peak * N {peak:.1f}"
    return (lambda: out.copy_(want.float().to(cx["dt"]).view(torch.int16))), check


def _dec_gn_finalize(st, o, cx):
    B, tiles, G = o.i[0], o.i[1], o.i[2]
    part = st.host(o.p[0], torch.float64, B, tiles, G, 2)
    want = torch.tensor([math.fsum(col) for col in part.permute(0, 2, 3, 1).reshape(-1, tiles).tolist()], dtype=torch.float64).view(B, G, 2)
    bound = tiles * 2.0 ** -53 * part.abs().sum(1)
    out = st.dst(o.p[1], torch.float64, 1, B * G * 2)

    def check():
        r, msg = worst("gn_finalize", out.cpu(), want, bound)
        assert msg is None, msg
        return "gn_finalize", r, f"({B}, {tiles}, {G})"
    return (lambda: out.copy_(want.view(1, -1))), check


def _dec_gn_act(st, o, cx):
    i, p, fl = o.i, o.p, o.flags
    B, HW, C, C2, G, eps = i[0], i[1], i[2], i[3], i[8] or 8, o.f[0]
    assert not (fl & ~(1 | 2 | 4)) and not C2 and not p[1] and not p[4] and not p[6] and not (i[5] or i[6] or i[7]), "a GroupNorm form this stepper does not restate"
    geo = nc.gn_geometry(B, HW, C, 0, G, fl)
    gname = cx["wname"][p[2]]
    assert gname.endswith(".weight") and cx["wname"][p[3]] == gname[:-7] + ".bias", "GroupNorm gain and bias of two layers"
    gamma, beta, silu = cx["vec"](p[2]), cx["vec"](p[3]), not (fl & 1)
    x = st.host(p[0], torch.float32, B, HW, C).double()
    read = st.host(p[7], torch.float64, B, G, 2)
    want, delta, sums, sums_bound = nc.gn_act_ref64(x, None, 1.0, G, gamma, beta, eps, nc.stat_counts(geo), silu=silu, stats=read if fl & 2 else None)
    n = HW * (C // G)
    var = sums[..., 1] / n - (sums[..., 0] / n) ** 2
    assert float(var.min()) > 0, f"{gname}: a group without variance"
    out = st.dst(p[5], torch.int16, B * HW, C)
    adds = geo["kernel"] in ("k_gn_stats_px", "k_gn_stats")
    stats = st.dst(p[7], torch.float64, 1, B * G * 2, prefill=False) if adds else None      # k_gn_one and flag 2 leave the buffer alone: the guard checks it

    def ref_write():
        out.copy_(want.float().to(cx["dt"]).view(torch.int16).view(B * HW, C))
        if adds:
            stats.copy_((read + sums).view(1, -1))

    def check():
        tag = f"{cx['tag']} {gname[:-7]} {geo['kernel']}"
        st_text = ""
        if fl & 2:          # the statistics the launch read are those of the tensor it normalises
            st_text = " statistics read " + _stats_ratio(tag, read, sums, sums_bound)
        elif adds:
            st_text = " statistics added " + _stats_ratio(tag, stats.cpu().view(B, G, 2) - read, sums, sums_bound)
        fig = nc.check_bf16(tag, out.cpu().view(cx["dt"]).view(B, HW, C), want, delta, log=False)
        inst = f"<{geo['NT']},{geo['NCH']}>" if geo["kernel"] == "k_gn_one" else ""
        return f"gn {geo['kernel']}{inst}", fig["worst"], f"{gname[:-7]} ({B}, {HW}, {C}) flags {fl} worst (err - half_ulp)/delta {fig['used']:.3f} mismatch {fig['mismatch']:.2e} median delta/half_ulp {fig['median']:.2e}{st_text}"
    return ref_write, check


def _dec_conv(st, o, cx):
    i, p, fl, dt = o.i, o.p, o.flags, cx["dt"]
    B, H, W, Cin, Ho, Wo, Cout, ldc, co_off, kh, kw, stride, pad, groups, tile = [i[j] for j in range(15)]
    groups = max(groups, 1)
    assert not (fl & ~(1 | 4 | 16 | 128)) and kh == kw and kh in (1, 3), "a conv form this stepper does not restate"
    assert (stride, pad) in ((1, kh // 2), (2, 0)) and (Ho, Wo) == ((H, W) if stride == 1 else (H // 2, W // 2))
    fam, twin, ups, M = conv_family(o), conv_has_twin(o), bool(fl & 16), B * Ho * Wo
    Hs, Ws = (H // 2, W // 2) if ups else (H, W)
    xs = st.host(p[0], torch.float32, B, Hs, Ws, Cin).to(dt) if fl & 1 else st.host(p[0], torch.int16, B, Hs, Ws, Cin).view(dt)
    xp = conv_input64(xs.double(), H, W, Ho, Wo, kh, stride, pad, ups)
    if p[1] in cx["wname"]:                  # a named layer: the module's parameter, rounded; input channels padded to the operand's width
        wn = cx["wname"][p[1]]
        w = cx["params"][wn]
        assert w.shape[0] == Cout and w.shape[1] <= Cin and w.shape[2:] == (kh, kw), f"{wn}: weight {tuple(w.shape)} for a {Cin} -> {Cout} {kh}x{kw} conv"
        w64 = torch.zeros(Cout, Cin, kh, kw, dtype=torch.float64)
        w64[:, :w.shape[1]] = w.to(dt).double()
    else:                                    # a per-sample GEMM on a device-packed activation: what the packed buffer holds
        assert B == 1 and kh == 1 and H == 1 and not p[2], "a packed-activation weight outside a per-sample GEMM"
        wn = "(packed)"
        buf = st.host(p[1], torch.int16, (Cout + 15) // 16 * (Cin // 32) * 512)
        w64 = unpack_weights(buf.data_ptr(), Cout, Cin, 1).double().view(Cout, Cin, 1, 1)
    bias = cx["vec"](p[2]).double() if p[2] else None
    if bias is not None:
        assert cx["wname"][p[2]] == wn[:-7] + ".bias", f"{wn}: the bias of another layer"
    assert not p[4] or (ldc == Cout and co_off == 0)
    resid = st.host(p[4], torch.float32, M, Cout).double() if p[4] else None
    row0 = p[3]              # rows of ldc floats start at p[3]; the op writes columns co_off .. co_off + Cout
    prev = st.host(row0, torch.float32, M, ldc)[:, co_off:co_off + Cout].double() if fl & 4 else None
    want, bound = conv_reference64(xp, w64, bias, prev, resid, stride, conv_chain(o), "cuda:0" if st.backend == "gpu" else "cpu")
    tight = float(bound.median()) / max(float(want.pow(2).mean().sqrt()), 1e-300)
    assert tight <= BOUND_MEDIAN_MAX, f"{wn}: median bound / rms = {tight:.2e}: the bound is too loose to see an error"
    out = st.dst(row0, torch.float32, M, Cout, ld=ldc, off=co_off, prefill=not (fl & 4))
    tw = st.dst(p[5], torch.int16, M, Cout) if twin else None
    if groups > 1:
        st.dst(p[5], torch.float32, 1, groups * M * ((Cout + 15) // 16 * 16))      # the split-K workspace
    cg = i[15]
    part = st.dst(p[6], torch.float64, M // 128, Cout // cg * 2) if fl & 128 else None
    assert not (fl & 128) or (cg in (4, 8, 16) and (Ho * Wo) % 128 == 0 and ldc == Cout)

    def ref_write():
        out.copy_(want.float())
        if tw is not None:
            tw.copy_(want.float().to(dt).view(torch.int16))
        if part is not None:
            part.copy_(tile_sums64(want.float().double(), cg, fam, B, Ho, Wo)[0].view(M // 128, -1))

    def check():
        got = out.cpu()
        r, msg = worst(f"conv {wn} ({fam}, tile {tile}, groups {groups})", got, want, bound)
        assert msg is None, msg
        if ldc != Cout:          # the pad lanes of the row: outside the destination (the guard) and exactly 0
            row = st.host(row0, torch.float32, M, ldc).view(torch.int32)
            row[:, co_off:co_off + Cout] = 0
            assert int(row.abs().max()) == 0, f"{wn}: a pad lane of the {ldc}-wide row is not exactly 0"
        if tw is not None:
            assert torch.equal(tw.cpu(), got.to(dt).view(torch.int16)), f"{wn}: the twin is not the rounding of the stored fp32 value"
        extra = ""
        if part is not None:
            sums, sb = tile_sums64(got.double(), cg, fam, B, Ho, Wo)
            rp, msg = worst(f"conv {wn}: epilogue partials", part.cpu().view(sums.shape), sums, sb)
            assert msg is None, msg
            extra = f" partials {rp:.3f}"
        return (f"conv {fam}{'+twin' if twin else ''}", r, f"{wn} ({B}, {H}x{W}, {Cin}->{Cout}) k {kh} s {stride} flags {fl} tile {tile} groups {groups} ldc {ldc} "
                f"c {conv_chain(o)} median bound / rms {tight:.1e}{extra}")
    return ref_write, check


_DECODERS = {(OP_MEMSET, 0): _dec_memset, (OP_ELTWISE, 2): _dec_pack_in, (OP_ELTWISE, 3): _dec_unpack_out, (OP_ELTWISE, 5): _dec_pack_act,
             (OP_ELTWISE, 6): _dec_softmax, (OP_GN_FINALIZE, 0): _dec_gn_finalize, (OP_GN_ACT, None): _dec_gn_act, (OP_CONV, None): _dec_conv}


# ---------------------------------------------------------------------------------------------------------------------------------
def check_wiring(plan, wname):
    """The dataflow of one plan, from the op records alone: which buffer an op must read is fixed by which op wrote it.  (A per-launch
    comparison cannot see an op that consistently reads the WRONG buffer.)
      * the trunk -- the tensor the next block reads -- is the output of the last conv_in / conv2 / proj_out / Downsample / Upsample /
        post_quant_conv; norm1, the AttnBlock's norm and norm_out read it, conv2's residual and proj_out's residual are the trunk their block
        started from;
      * a GroupNorm with flag 2 reads the statistics the OP_GN_FINALIZE right before it wrote, from the partials of the conv that last wrote
        that GroupNorm's input, in groups of the GroupNorm's width;
      * an Upsample, Downsample or nin_shortcut reads the trunk or the twin of the conv that wrote it;
      * each per-sample attention GEMM reads the packed operand the ELTWISE 5 of the same sample wrote, from that sample's rows of k / v."""
    ops = plan.ops
    writer, twin_of, trunk, block_in, outs = {}, {}, None, None, {}
    pack, scores, probs, gn_out = {}, {}, {}, {}
    name_of = lambda o: wname.get(o.p[1], "")[:-7]          # noqa: E731  layer name of a conv with a named weight
    for k, o in enumerate(ops):
        if o.type == OP_GN_ACT:
            g = wname[o.p[2]][:-7]
            gn_out[g] = o.p[5]
            if g.endswith((".norm1", ".norm", "norm_out")):
                assert o.p[0] == trunk, f"{g} does not read the block input"
                block_in = trunk
            else:
                assert g.endswith(".norm2") and writer[o.p[0]] is outs[g[:-6] + ".conv1"], f"{g} does not read conv1 of its block"
            if o.flags & 2:
                fin, conv = ops[k - 1], writer[o.p[0]]
                assert fin.type == OP_GN_FINALIZE and fin.p[1] == o.p[7] and (fin.i[0], fin.i[1] * 128, fin.i[2]) == (o.i[0], o.i[1], o.i[8]), f"{g}: not the statistics of the OP_GN_FINALIZE before it"
                assert conv.type == OP_CONV and (conv.flags & 128) and conv.p[6] == fin.p[0] and conv.i[15] == o.i[2] // o.i[8] and conv.i[6] == o.i[2], \
                    f"{g}: the partials are not those of the conv that wrote its input"
        elif o.type == OP_ELTWISE and o.flags == 5:
            pack[o.p[3]] = o
        elif o.type == OP_ELTWISE and o.flags == 6:
            assert o.p[0] in scores, "a softmax of something no q.k^T GEMM wrote"
            probs[o.p[3]] = scores[o.p[0]]
        elif o.type == OP_ELTWISE and o.flags == 2:
            writer[o.p[3]] = o
        elif o.type == OP_CONV:
            n = name_of(o)
            if not n:                                    # a per-sample GEMM of the AttnBlock
                pk = pack.get(o.p[1])
                assert pk is not None, "a per-sample GEMM whose B operand no ELTWISE 5 wrote"
                HW, C = (o.i[6], o.i[3]) if o.flags & 1 else (o.i[3], o.i[6])
                q, kk, v = (outs[f"{attn_block}.{t}"] for t in "qkv")
                if o.flags & 1:                          # S = q K^T of sample b
                    b, rem = divmod(o.p[0] - q.p[3], HW * C * 4)
                    assert rem == 0 and 0 <= b < plan.B and pk.i[3] == 0 and pk.p[0] == kk.p[3] + b * HW * C * 4, "q.k^T: not the packed k of the same sample"
                    scores[o.p[3]] = b
                else:                                    # out = P V of sample b
                    b = probs.get(o.p[0])
                    assert b is not None and pk.i[3] == 1 and pk.p[0] == v.p[3] + b * HW * C * 4, "P.v: not the probabilities and the packed v of the same sample"
                    if b == 0:
                        att = o.p[3]
                    assert o.p[3] == att + b * HW * C * 4, "P.v: not that sample's rows of the attention output"
                continue
            src = o.p[0]
            if n.endswith(("downsample.conv", "upsample.conv", ".nin_shortcut")):
                assert src == trunk or (src == twin_of.get(trunk) and not (o.flags & 1)), f"{n} reads neither the block input nor the twin of the conv that wrote it"
            elif n.endswith(".proj_out"):
                assert src == att and o.p[4] == block_in and (o.flags & 1), f"{n}: not the attention output plus the block input"
            elif n.endswith((".q", ".k", ".v")):
                attn_block = n[:-2]
            elif n == "quant_conv":
                assert src == outs["encoder.conv_out"].p[3] and (o.flags & 1), "quant_conv does not read the moment rows"
            elif n == "decoder.conv_in":
                assert src == trunk and (o.flags & 1), "decoder.conv_in does not read the post_quant_conv rows"
            for suffix, norm in ((".conv1", ".norm1"), (".conv2", ".norm2"), (".q", ".norm"), (".k", ".norm"), (".v", ".norm"), (".conv_out", ".norm_out")):
                if n.endswith(suffix):
                    assert src == gn_out.get(n[:-len(suffix)] + norm) and not (o.flags & 1), f"{n} does not read the output of its GroupNorm"
            if n.endswith(".conv2"):
                assert bool(o.p[4]) != bool(o.flags & 4) and (o.p[4] == block_in or writer[o.p[3]] is outs[n[:-6] + ".nin_shortcut"]), f"{n}: the residual is not the block input"
            outs[n] = o
            writer[o.p[3]] = o
            if conv_has_twin(o):
                twin_of[o.p[3]] = o.p[5]
            if n.endswith(("conv_in", ".conv2", ".proj_out", "downsample.conv", "upsample.conv", "post_quant_conv")):
                trunk = o.p[3]
    last = ops[-1]
    assert last.type == OP_ELTWISE and last.flags == 3 and last.p[3] == plan.out.ptr and writer.get(last.p[0]) is not None, "the plan's output is not unpacked from a conv output"


# ---------------------------------------------------------------------------------------------------------------------------------
# the exception kinds, at a small size: the tile code of an op record selects the 128-channel tile at any M
EXCEPTION_OPS = {          # canonical kind -> (flags, k, stride, Cin, H): one image, 128 output channels in groups of 4, M = 256
    ("conv", 128, "glds", False, 3, 2, 8, False, False): (128, 3, 2, 64, 32),
    ("conv", 128, "glds", True, 3, 2, 8, False, False): (128, 3, 2, 64, 32),
    ("conv", 129, "lds", False, 1, 1, 8, False, False): (129, 1, 1, 64, 16),
}


def run_exception_case(kind, backend="gpu"):
    """One hand-built op of an EXCEPTIONS kind through the same decoder, references and guard as a plan's launches."""
    from types import SimpleNamespace
    flags, k, stride, Cin, H = EXCEPTION_OPS[kind]
    dev = torch.device(device_of(backend))
    dt = _lib.operand_dtype(_lib.lib())
    Cout, cg, Ho = 128, 4, H // stride
    M = Ho * Ho
    g = torch.Generator().manual_seed(Cin + H + k)
    w, bias = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5, torch.randn(Cout, generator=g)
    x = torch.randn(1, H, H, Cin, generator=g) + 0.3
    wp, cpad = nc.pack_conv(w, dev)
    assert cpad == Cin
    bd = bias.to(dev)
    sizes = [H * H * Cin * 4, M * Cout * 4, M * Cout * 2, M // 128 * (Cout // cg) * 2 * 8]          # A (room for fp32), out, twin, partials
    offs = [sum((n + 255) // 256 * 256 + 256 for n in sizes[:j]) + 256 for j in range(4)]           # a gap between the buffers: the guard sees an overrun
    arena = torch.full((offs[-1] + sizes[-1] + 512,), 0x5a, dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    a_ptr, out_ptr, tw_ptr, part_ptr = (base + o for o in offs)
    mem = lc._Mem([SimpleNamespace(zero=SimpleNamespace(buf=None), misc=SimpleNamespace(buf=arena))])
    if flags & 1:
        mem.view(a_ptr, torch.float32, 1, H, H, Cin).copy_(x)
    else:
        mem.view(a_ptr, torch.int16, 1, H, H, Cin).copy_(x.to(dt).view(torch.int16))
    o = nc.mkop(OP_CONV, flags, p=(a_ptr, wp, bd, out_ptr, None, tw_ptr if kind[3] else None, part_ptr),
                i=(1, H, H, Cin, Ho, Ho, Cout, Cout, 0, k, k, stride, (k // 2 if stride == 1 else 0), 1, 256 + 8, cg))
    assert launch_kind(o) == kind, launch_kind(o)
    label, r, text = step_op(mem, backend, o, dict(tag=f"exception {kind}", dt=dt, wname={wp.data_ptr(): "t.weight", bd.data_ptr(): "t.bias"},
                                                   params={"t.weight": w, "t.bias": bias}, attn_peaks=[]))
    print(f"margin exception {kind} {label} err / bound {r:.3f}  {text}")

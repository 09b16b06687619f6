"""Launch-plan machinery shared by every model on the HIP op set (csrc/unet_ops.hip): the op codes, the two device arenas, planned
tensors with their lazy / slots / twin state, the split-K workspaces and the generic emitters (conv, gn_act, ln, gemv, attn).  A model
subclasses `Plan` with its own layer logic (unet._Plan, vae._VaePlan, lpips._LpipsPlan, eft._EftPlan); its owner module inherits
`PlanOwner`, which declares every switch these emitters read and the implicit-GEMM cost model."""
import torch

from . import _lib

OP_CONV, OP_GN_ACT, OP_LN, OP_GEMV, OP_ATTN, OP_GCA_POOL, OP_ELTWISE, OP_MEMSET, OP_TIME_EMB, OP_SPLITK_REDUCE = range(1, 11)
OP_FCONV, OP_SLOTS, OP_GCA, OP_INITX, OP_GN_FINALIZE = 14, 15, 16, 17, 18
FNORM_NONE, FNORM_GN_SELF, FNORM_GN_SLOTS, FNORM_LN, FNORM_ATTN = range(5)      # csrc/fused_kernels.h
LDS_MAX = 163840
SKIP_SCALE = 2 ** -0.5            # scale_skip_connection (imagen_pytorch.py:1283)


class _Arena:
    """Bump allocator over one device tensor.  `base=None` = sizing pass (offsets only)."""

    def __init__(self, nbytes=None, device=None):
        self.off = 0
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None

    def alloc(self, nbytes):
        nbytes = (nbytes + 255) // 256 * 256
        off = self.off
        self.off += nbytes
        return (self.buf.data_ptr() + off) if self.buf is not None else (1 << 20) + off


class _T:
    """A planned activation: device pointer + logical shape [B, HW, C] (NHWC) or [rows, C]."""
    __slots__ = ("ptr", "rows", "C", "HW", "lazy", "slots", "writer", "twin")

    def __init__(self, ptr, rows, C, HW=None):
        self.ptr, self.rows, self.C, self.HW = ptr, rows, C, HW
        # lazy: None, or how the first consumer must materialise the tensor (csrc/unet_ops.hip LazySrc):
        #   ("splitk", ws, bias, resid, groups, npad, ws index)   or   ("gate", h, gate, res)
        self.lazy = None
        # slots: device pointer of the [rows/16][C/16][2] (sum, sum of squares) table of the materialised values that a
        # GroupNorm-fused conv reads its statistics from (csrc/fused_kernels.h), or None
        self.slots = None
        self.twin = None            # operand-type copy [rows][C] written by the producing conv's epilogue (Plan.conv twin=), or None
        # writer: the OP_CONV op (k_conv_lds) that wrote the whole tensor last, or None (experimental GroupNorm-partials epilogue)
        self.writer = None


class PlanOwner:
    """Mixin of a module that owns launch plans (`Plan.u`): the switches the generic emitters read, with the value a plain owner
    means.  An owner overrides what it needs as class or instance attributes and provides `_packed(device)`."""
    conv_waves_target = 1024        # waves wanted per conv launch (4 per CU) before split-K stops
    lds_conv_min_blocks = 0         # use k_conv_lds when a layer has at least this many 128 x 128 output tiles; 0 = never
    lds_mid_min_rows = 0            # convs of >= this many rows with too few tiles for lds_conv_min_blocks run LDS-tiled with split-K groups; 0 = off
    lds_mid_min_batch = 8           # ... in plans of at least this many images
    gn_epilogue = False             # GroupNorm statistics out of the producing k_conv_lds epilogue instead of a pass over the tensor
    gn_one = True                   # GroupNorm passes in one launch (k_gn_one) where it fits; False: k_gn_stats + k_gn_apply everywhere
    ln_wave = True                  # LayerNorm of <= 256 rows of 512 | 1024 | 2048 channels on k_layernorm_wave (False: op flag 4 = k_layernorm)
    tb_stride = 0                   # floats per row of the time block a GroupNorm reads its (scale, shift) from; 0 = none
    lazy_consumers = 0              # bit 0: split-K reductions, bit 1: gated residuals are materialised by their first consumer
    ss_total = 0                    # width of the batched time-MLP output ((scale, shift) of every block); 0 = no time path
    igemm_t = 0                     # bit j: the launch whose geometry is row j of igemm_t_variants runs on k_conv_igemm_t (op flag 512); 0 = never
    igemm_t_variants = ()           # the rows of csrc/conv_igemm_t.h SF_IGEMM_T_VARIANTS, in its order (UNet only)
    tile_override = None            # {(m_frags, n_frags, KS, pixshuf): (WM, WN, groups)}: measured picks that replace the cost model (UNet only)

    def conv_tiling(self, m_frags, n_frags, KS, pixshuf=False):
        """(WM, WN, split-K groups) of one implicit-GEMM launch, by a small cost model.  A wave owns a
        (16*WM x 16*WN) tile; the 4 waves of a workgroup split K four ways (reduced in LDS); `groups` further K
        slices go through the workspace + k_splitk_reduce.  Terms: weight streaming from HBM (needs ~4 waves/CU
        to saturate), fragment traffic from L2 (1 KiB per fragment, amortised over the tile), MFMA issue, and the
        partial-tile round trip of split-K."""
        ov = self.tile_override                                 # measured picks (unet.TILE_PICKS) and tools/tile_sweep.py
        if ov and (m_frags, n_frags, KS, bool(pixshuf)) in ov:
            return ov[(m_frags, n_frags, KS, bool(pixshuf))]
        best = None
        mfma = m_frags * n_frags * KS
        w_bytes = n_frags * KS * 1024
        for WM in (1, 2, 4):
            if m_frags % WM or (m_frags <= 4 and WM != m_frags and m_frags in (1, 2, 4)):
                continue                                   # small maps: all rows in one tile -> weights fetched once
            for WN in (1, 2, 4):
                if n_frags % WN:
                    continue
                tiles = (m_frags // WM) * (n_frags // WN)
                for groups in ((1,) if pixshuf else (1, 2, 4, 8, 16, 32)):
                    if groups > 1 and KS // (4 * groups) < 2:
                        continue
                    waves = tiles * groups * 4
                    util = min(1.0, waves / self.conv_waves_target)
                    t_hbm = w_bytes / 4.0e12 / util
                    t_l2 = mfma * 1024 * (1.0 / WN + 1.0 / WM) / 12.0e12 / util
                    t_mfma = mfma * 20 / (1024 * 2.1e9) / util
                    t_part = (2.0 * groups * m_frags * n_frags * 1024 / 3.0e12 + 2.0e-6) if groups > 1 else 0.0
                    cost = max(t_hbm, t_l2, t_mfma) + t_part + 1e-9 * WM * WN
                    if best is None or cost < best[0]:
                        best = (cost, WM, WN, groups)
        return best[1], best[2], best[3]


class Plan:
    """Base of a model's static launch plan: `u` is the owning module (a PlanOwner), `sizing=None` the sizing pass."""

    def __init__(self, unet, B, device, sizing=None):
        self.u, self.B, self.dev = unet, B, device
        self.ops = []
        self.graph = None
        if sizing is None:
            self.zero, self.misc = _Arena(), _Arena()
        else:
            self.zero, self.misc = _Arena(sizing[0], device), _Arena(sizing[1], device)
        self.w = unet._packed(device)
        self.written = set()                 # (ptr, channel offset) of conv outputs that already hold data
        # two split-K workspaces (max demand over the ops that use each; ops run serially): a fused conv reads its input's
        # slabs from one while it writes its own partial tiles to the other
        self.ws_need = [0, 0]
        self.ws_ptrs = [self.misc.alloc(sizing[2]) if sizing is not None else 0,
                        self.misc.alloc(sizing[3]) if sizing is not None and len(sizing) > 3 and sizing[3] else 0]
        self.ws_owners = [None, None]        # tensors whose un-reduced split-K partials currently live in each workspace

    @property
    def ws_bytes(self):
        return self.ws_need[0]

    @property
    def ws2_bytes(self):
        return self.ws_need[1]

    @property
    def ws_owner(self):
        return next((o for o in self.ws_owners if o is not None and o.lazy is not None), None)

    def acquire_ws(self, nbytes, avoid=()):
        """Index of a workspace the op being emitted may overwrite: a free one if possible, never one that holds the
        partials of a tensor in `avoid` (an input of that op); a workspace owned by another tensor is reduced first."""
        for i in sorted(range(2), key=lambda j: (self.ws_owners[j] is not None and self.ws_owners[j].lazy is not None, j)):
            o = self.ws_owners[i]
            if o is not None and o.lazy is not None:
                if any(o is t for t in avoid):
                    continue
                self.need(o)
            self.ws_need[i] = max(self.ws_need[i], nbytes)
            self.ws_owners[i] = None
            return i
        raise AssertionError("no split-K workspace available")

    # -------- allocation helpers
    def f32(self, rows, C, HW=None):
        return _T(self.misc.alloc(rows * C * 4), rows, C, HW)

    def bf16(self, rows, C, HW=None):
        return _T(self.misc.alloc(rows * C * 2), rows, C, HW)

    def op(self, type_, flags=0, p=(), i=(), f=()):
        o = _lib.SfOp()
        o.type, o.flags = type_, flags
        for k, v in enumerate(p):
            o.p[k] = v if v else None
        for k, v in enumerate(i):
            o.i[k] = int(v)
        for k, v in enumerate(f):
            o.f[k] = float(v)
        self.ops.append(o)

    def wptr(self, name):
        return self.w[name].data_ptr()

    # -------- lazy tensors: the first consumer materialises them (saves one dependent launch each)
    def need(self, t):
        """Emit the stand-alone materialisation of a lazy tensor for consumers that cannot do it themselves."""
        if t is None or t.lazy is None:
            return t
        lz, t.lazy = t.lazy, None
        if lz[0] == "splitk":
            _, ws, bias, resid, groups, npad, wi = lz
            self.op(OP_SPLITK_REDUCE, 0, p=(ws, bias, resid, t.ptr), i=(t.rows, t.C, npad, groups))
            self.ws_owners[wi] = None
        else:
            _, h, gate, res = lz
            self.op(OP_ELTWISE, 1, p=(h, gate, res, t.ptr), i=(self.B, t.HW, t.C))
        return t

    def take_lazy(self, t, allow):
        """(p[8..10], (mode, groups, npad)) for a consumer that materialises `t` itself; clears the lazy state."""
        if t.lazy is None or t.lazy[0] not in allow:
            self.need(t)
            return (0, 0, 0), (0, 0, 0)
        lz, t.lazy = t.lazy, None
        if lz[0] == "splitk":
            self.ws_owners[lz[6]] = None
            return (lz[1], lz[2], lz[3]), (1, lz[4], lz[5])
        return (lz[1], lz[2], lz[3]), (2, 0, 0)

    # -------- op emitters
    def conv(self, x, x_f32, H, W, wname, bname, out, ldc, co_off, Cout, k, stride=1, pad=0, resid=None, pixshuf=False,
             defer=False, w_ptr=None, batch=None, out_hw=None, upsampled=False, relu=False, gelu=False, twin=None, want_slots=False,
             nchw=False, defer_max_groups=8):
        """One implicit-GEMM launch.  `w_ptr` replaces the named weight by a device-packed B operand (attention),
        `batch` overrides the plan batch (per-sample GEMMs), `out_hw` the output size (asymmetric padding),
        `upsampled` makes (H, W) the dims of a nearest-x2 view of the stored [H/2, W/2] input.  `twin`: a dense operand-type
        [M][Cout] buffer the epilogue of an LDS-tiled kernel also fills (the A operand of a following conv: no fp32 round trip);
        out.twin is set when the chosen kernel writes it."""
        B = self.B if batch is None else batch
        self.need(x)
        self.need(resid)
        Ho, Wo = out_hw or ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)
        M = B * Ho * Wo
        m_frags, n_frags = (M + 15) // 16, (Cout + 15) // 16
        KS = k * k * (x.C // 32)
        WM, WN, groups = self.u.conv_tiling(m_frags, n_frags, KS, pixshuf)
        accum = (out.ptr, co_off) in self.written
        self.written.add((out.ptr, co_off))
        tile = WM * 16 + WN
        twin_ws = 0
        # large-M layers (VAE, VGG, B >= 4): the LDS-tiled kernel, 128 pixels x 128 (or 64) channels per workgroup
        lds_min = self.u.lds_conv_min_blocks
        mid = self.u.lds_mid_min_rows if B >= self.u.lds_mid_min_batch else 0
        if lds_min and n_frags >= 4 and (not pixshuf or (mid and M >= mid and Cout % 4 == 0)):
            bnf = 8 if n_frags > 4 else 4
            blocks = ((m_frags + 7) // 8) * ((n_frags + bnf - 1) // bnf)
            if bnf == 8 and blocks < 256:                     # fewer tiles than CUs: halve the channel tile instead of idling CUs
                bnf, blocks = 4, ((m_frags + 7) // 8) * ((n_frags + 3) // 4)
            # 3x3 layers k_conv3_halo takes (csrc/conv_halo.h) beat the weight-streaming kernel from 64 tiles on (measured 21 vs 29 us
            # on the 32x32 512->512 layer); everything else needs lds_min tiles
            halo = (k == 3 and stride == 1 and pad == 1 and not x_f32 and x.C % 64 == 0 and W % 16 == 0 and H % 8 == 0 and M % 128 == 0
                    and Cout % 4 == 0 and ldc % 4 == 0 and co_off % 4 == 0 and (Ho, Wo) == (H, W) and not pixshuf)
            if blocks >= (min(lds_min, 64) if halo else lds_min) and not pixshuf:
                tile, groups = 256 + bnf, 1
                if twin is not None and ldc == Cout and co_off == 0:
                    twin_ws = twin.ptr
            elif mid and M >= mid:
                # r06: M of a few hundred rows (the 4x4 level of B >= 8, the Upsample 1x1 convs): still 128-row MFMA tiles out of LDS, the
                # workgroups that are missing come from split-K groups over the stage range (k_conv_lds / k_conv_glds; not under the
                # pixel shuffle, whose epilogue writes the output itself) -- every weight byte is still fetched by ONE workgroup per pixel tile
                glds_ok = not x_f32 and x.C % 64 == 0 and Cout % 4 == 0 and ldc % 4 == 0 and co_off % 4 == 0
                stages = KS // 2 if glds_ok else (KS + 1) // 2
                g = 1 if pixshuf else max(1, min(256 // blocks, stages // 4, 16))
                if glds_ok and k == 3 and stride == 1 and pad == 1 and H == W and H in (4, 8) and not pixshuf:
                    # whole 4x4 / 8x8 maps: k_conv3_halo_sm (csrc/conv_halo_small.h) splits K by 64-channel chunk, two chunks per group at least
                    # (the frames of the second are staged under the taps of the first)
                    g = max(1, min(256 // blocks, x.C // 128, 16))
                tile, groups = 256 + bnf, g
        ws, wi = 0, 0
        if groups > 1:
            wi = self.acquire_ws(groups * M * n_frags * 16 * 4)   # a workspace about to be overwritten is reduced first
            ws = self.ws_ptrs[wi]
        elif twin_ws:
            ws = twin_ws
        defer = bool(defer and not relu and not gelu and 1 < groups <= defer_max_groups and not accum and not pixshuf and co_off == 0 and ldc == Cout == out.C and M == out.rows
                     and (self.u.lazy_consumers & 1))
        bias, res = self.wptr(bname) if bname else 0, resid.ptr if resid else 0
        # r04: the SiLU + PixelShuffle epilogue of an Upsample also leaves the (sum, sum of squares) slots of its output for the next
        # GroupNorm-fused conv (was a k_slots launch): one slot per MFMA fragment, filed under the right (image, 16-channel column)
        slots = 0
        if want_slots and pixshuf and tile < 256 and (Cout // 4) % 16 == 0 and ldc % 16 == 0 and co_off % 16 == 0 and (Ho * Wo) % 16 == 0 and not accum:
            slots = self.misc.alloc(4 * M // 16 * (ldc // 16) * 2 * 4)
        # nchw: the (non-deferred) split-K reduction of this conv writes the plan's NCHW output directly (was k_unpack_out)
        nchw = bool(nchw and groups > 1 and not defer and not accum and not resid and tile < 256 and co_off == 0 and ldc == Cout)
        # k_conv_igemm_t (csrc/conv_igemm_t.h): a one-image launch whose whole geometry is a row of the variant table; the host checks the
        # same conditions and keeps k_conv_igemm for anything else
        igt = False
        if self.u.igemm_t and tile < 256 and B == 1 and H == W and (Ho, Wo) == ((H + 2 * pad - k) // stride + 1,) * 2 and not (accum or res or relu or gelu or co_off):
            key = (H.bit_length() - 1, x.C, Cout, k, stride, pad, int(bool(upsampled)), WM, WN, groups, int(bool(x_f32)), 1 if pixshuf else 0)
            if key in self.u.igemm_t_variants and H == 1 << key[0] and (self.u.igemm_t >> self.u.igemm_t_variants.index(key)) & 1:
                igt = bool(slots and bias and ldc * 4 == Cout) if pixshuf else groups > 1
        self.op(OP_CONV, (1 if x_f32 else 0) | (2 if pixshuf else 0) | (4 if accum else 0) | (8 if defer else 0) |
                (16 if upsampled else 0) | (32 if relu else 0) | (64 if gelu else 0) | (256 if nchw else 0) | (512 if igt else 0),
                p=(x.ptr, w_ptr if w_ptr is not None else self.wptr(wname), bias, out.ptr, res, ws, 0, slots),
                i=(B, H, W, x.C, Ho, Wo, Cout, ldc, co_off, k, k, stride, pad, groups, tile))
        if defer:
            out.lazy = ("splitk", ws, bias, res, groups, n_frags * 16, wi)
            self.ws_owners[wi] = out
        out.slots = slots or None
        self.last_conv_nchw = nchw
        out.writer = self.ops[-1] if (tile >= 256 and co_off == 0 and ldc == Cout == out.C and M == out.rows) else None
        out.twin = twin if (twin is not None and tile >= 256 and groups == 1 and ws == twin.ptr) else None
        return Ho, Wo

    def gn_act(self, x, skip, gname, ss_ptr, out, raw=None, silu=True, groups=8, eps=1e-5):
        C1, C2 = x.C, (skip.C if skip else 0)
        self.need(skip)
        lp, li = self.take_lazy(x, ("splitk", "gate"))
        stats = self.zero.alloc(self.B * groups * 2 * 8)     # f64 (sum, sum of squares) per (b, group), zeroed per eval
        ready = 0
        wr = x.writer
        cg = (C1 // groups) if not skip else 0
        if (self.u.gn_epilogue and wr is not None and not (wr.flags & 128) and li[0] == 0 and cg in (4, 8, 16)
                and x.HW and x.HW % 128 == 0 and x.rows == self.B * x.HW):
            # (VAE plans; SF_VAE_GN_EPI=0 disables) the producing k_conv_lds leaves per-tile partial sums, k_gn_finalize adds them up,
            # and the statistics pass over the tensor (k_gn_stats_px) is skipped
            part = self.misc.alloc(x.rows // 128 * groups * 2 * 8)
            wr.flags |= 128
            wr.p[6] = part or None
            wr.i[15] = cg
            self.op(OP_GN_FINALIZE, 0, p=(part, stats), i=(self.B, x.HW // 128, groups))
            ready = 2
        self.op(OP_GN_ACT, (0 if silu else 1) | ready | (0 if self.u.gn_one else 4),      # (flag 4: k_gn_stats + k_gn_apply even where k_gn_one fits)
                p=(x.ptr, skip.ptr if skip else 0, self.wptr(gname + ".weight"), self.wptr(gname + ".bias"), ss_ptr, out.ptr,
                   raw.ptr if raw else 0, stats) + lp,
                i=(self.B, x.HW, C1, C2, self.u.tb_stride) + li + (groups,), f=(eps, SKIP_SCALE))

    def ln(self, x, gname, bname, out, C, rows, eps=1e-5, gelu=False, out_f32=False, resid=None, twin=None):
        """`twin`: an operand-type [rows][C] buffer that also receives the (fp32-output) result -- the A operand of the next linear
        (k_layernorm_w256: C = 256, rows >= 1024 only)."""
        self.need(x)
        self.need(resid)
        assert twin is None or (out_f32 and C == 256 and rows >= 1024)
        self.op(OP_LN, (1 if gelu else 0) | (2 if out_f32 else 0) | (0 if self.u.ln_wave else 4),
                p=(x.ptr, self.wptr(gname), self.wptr(bname) if bname else 0, out.ptr, resid.ptr if resid else 0, twin.ptr if twin else 0),
                i=(rows, C), f=(eps,))
        out.twin = twin

    def gemv(self, x_ptr, M, ldx, wname, bname, y_ptr, ldy, N, K, in_silu=False, out_act=0):
        Kp = (K + 7) // 8 * 8
        # > 8 rows (a sampler's time table): k_gemm_rows, up to 64 rows per launch 
        step = 8 if M <= 8 else 64
        for m0 in range(0, M, step):
            mm = min(step, M - m0)
            self.op(OP_GEMV, (1 if in_silu else 0) | (out_act << 1),
                    p=(x_ptr + m0 * ldx * 4, self.wptr(wname), self.wptr(bname) if bname else 0, y_ptr + m0 * ldy * 4),
                    i=(mm, N, K, Kp, ldx, ldy))

    def attn(self, q, out, segs, heads, ldq, scale, out_f32=False):
        p = [q.ptr, out.ptr]
        i = [self.B, heads, ldq, 0]
        for s in (segs + [None] * 3)[:3]:
            if s is None:
                p += [0, 0]
                i += [0, 0, 0, 0]
            else:
                p += [s[0], s[1]]
                i += list(s[2:])
        self.op(OP_ATTN, 1 if out_f32 else 0, p=p, i=i, f=(scale,))

    def tview(self, t):
        """torch view of a planned fp32 buffer of the misc arena (static input / output staging)."""
        off = t.ptr - self.misc.buf.data_ptr()
        return self.misc.buf[off:off + t.rows * t.C * 4].view(torch.float32).view(t.rows, t.C)

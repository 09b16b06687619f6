"""One SHA-256 per launch plan, built in sizing mode on the CPU (no GPU): the check of a planner refactor.  Run it at two commits and
diff the outputs -- equal lines mean the plans are the same op for op (type, flags, i[], f[], p[] of every SfOp, zero.off, misc.off and
the split-K workspace demand), hence the same GPU work.  Sizing-mode pointers are arena offsets; pointers into a packed weight differ
between processes and are hashed as (weight name, byte offset); any other pointer is an error, never hashed.

Covers the canonical / dim-64 / dim-128 UNets at twelve batch sizes, every entry of unet.SWITCHES changed singly at B = 1, 4, 16
(booleans flipped, numbers set to 0, lazy_consumers 0 .. 3, the "r05" plan of tests/test_gpu_unet.py), the time-table plans, and the
VAE / LPIPS / EFT plans of tests/test_plans_cpu.py with their own switches on and off.
usage: plan_digest.py [--switches a,b,c]      (--switches: the names to vary, for a tree that has no unet.SWITCHES table yet)"""
import bisect
import hashlib
import os
import struct
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import unet_ref                                                  # noqa: E402
from sparsefusion_amd import unet as U                                       # noqa: E402
from sparsefusion_amd.eft import EpipolarFeatureTransformer, _EftPlan        # noqa: E402
from sparsefusion_amd.lpips import LPIPS, _LpipsPlan                         # noqa: E402
from sparsefusion_amd.vae import AutoencoderKL, _VaePlan                     # noqa: E402

CPU = torch.device("cpu")
ARENA_BASE = 1 << 20                         # what a sizing-mode arena hands out (plan._Arena.alloc)
BATCHES = (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 24, 32)


def digest(plan, extra_ops=(), arenas=(), tensors=()):
    """`arenas`: earlier plans whose buffers this one reads (LPIPS backward, EFT forward); `tensors`: (name, tensor) of caller inputs."""
    known = sorted((t.data_ptr(), t.data_ptr() + max(1, t.numel() * t.element_size()), name)
                   for name, t in list(plan.w.items()) + list(tensors))
    starts = [k[0] for k in known]
    limit = ARENA_BASE + max(max(p.zero.off, p.misc.off) for p in (plan,) + tuple(arenas))
    h = hashlib.sha256()

    def pointer(v, o, k):
        if not v:
            return b"null"
        j = bisect.bisect_right(starts, v) - 1
        if j >= 0 and v < known[j][1]:
            return f"{known[j][2]}+{v - known[j][0]}".encode()
        if ARENA_BASE <= v < limit:
            return f"arena+{v - ARENA_BASE}".encode()
        if v == 1 and o.type == U.OP_MEMSET and k == 0:      # the sizing pass's stand-in for the base of the zero arena
            return b"zero-arena"
        raise SystemExit(f"plan_digest: op type {o.type} p[{k}] = {v:#x} is neither an arena offset nor inside a known tensor")

    ops = list(plan.ops) + list(extra_ops)
    for o in ops:
        h.update(struct.pack("<2i32i8f", o.type, o.flags, *o.i, *o.f))
        for k, v in enumerate(o.p):
            h.update(pointer(v, o, k) + b";")
    h.update(struct.pack("<4q", plan.zero.off, plan.misc.off, *plan.ws_need))
    return f"{h.hexdigest()} ops={len(ops)}"


def unet_digest(net, B):
    plan = U._Plan(net, B, CPU).build()
    h = hashlib.sha256(digest(plan, extra_ops=plan.init_x_ops).encode())
    h.update(struct.pack("<2q", plan.n_time_ops, plan.n_init_ops))
    return f"{h.hexdigest()} ops={len(plan.ops)}+{len(plan.init_x_ops)}"


def variants(names, net):
    """(label, {attribute: value}) for every switch changed singly."""
    for name in names:
        default = getattr(net, name)
        if name == "lazy_consumers":
            values = [v for v in (0, 1, 2, 3) if v != default]
        elif name == "conv_waves_target":
            values = [default // 2]                          # a divisor of the cost model, not a threshold: 0 has no meaning
        elif isinstance(default, bool):
            values = [not default]
        else:
            values = [0] if default else [1]
        for v in values:
            yield f"{name}={int(v)}", {name: v}
    yield "r05", {"lds_mid_min_rows": 0, "unfused_min_rows_4": 0, "unfused_min_rows_8": 0}
    yield "tile_override={}", {"tile_override": {}}


def main():
    names = [n for n, *_ in getattr(U, "SWITCHES", ())]
    if "--switches" in sys.argv:
        names = sys.argv[sys.argv.index("--switches") + 1].split(",")
    assert names, "no unet.SWITCHES in this tree: pass --switches name,name,..."
    for cname, cfg in (("canonical", unet_ref.CANONICAL), ("dim64", unet_ref.SMALL), ("dim128", unet_ref.MEDIUM)):
        net = U.Unet(**cfg, layer_cross_attns=(False,) * 4, attn_pool_text=False)
        for B in BATCHES:
            print(f"unet {cname} B={B}: {unet_digest(net, B)}", flush=True)
        if cname != "canonical":
            continue
        for label, attrs in variants(names, net):
            saved = {k: getattr(net, k) for k in attrs}
            for k, v in attrs.items():
                setattr(net, k, v)
            for B in (1, 4, 16):
                print(f"unet canonical {label} B={B}: {unet_digest(net, B)}", flush=True)
            for k, v in saved.items():
                setattr(net, k, v)
        for T in (51, 100):
            print(f"unet time table T={T}: {digest(U._TimePlan(net, T, CPU).build())}", flush=True)
    for conv_twin in (True, False):
        for gn_epilogue in (True, False):
            vae = AutoencoderKL()
            vae.conv_twin, vae.gn_epilogue = conv_twin, gn_epilogue
            for kind, B in (("enc", 1), ("dec", 1), ("dec", 2)):
                print(f"vae {kind} B={B} conv_twin={int(conv_twin)} gn_epilogue={int(gn_epilogue)}: "
                      f"{digest(_VaePlan(vae, kind, B, CPU).build())}", flush=True)
    for conv_twin in (True, False):
        lp = LPIPS()
        lp.conv_twin = conv_twin
        fwd = _LpipsPlan(lp, 1, 256, CPU).build_forward()
        print(f"lpips fwd conv_twin={int(conv_twin)}: {digest(fwd)}", flush=True)
        bwd = _LpipsPlan(lp, 1, 256, CPU, fwd=fwd).build_backward()
        print(f"lpips bwd conv_twin={int(conv_twin)}: {digest(bwd, arenas=(fwd,))}", flush=True)
    images = torch.zeros(6, 3, 256, 256)
    for linear_twin in (True, False):
        eft = EpipolarFeatureTransformer(use_r=True, encoder='resnet18', return_features=True, remove_unused_layers=False)
        eft.linear_twin = linear_twin
        enc = _EftPlan(eft, 6, CPU).build_encoder(6, 256)
        print(f"eft enc linear_twin={int(linear_twin)}: {digest(enc)}", flush=True)
        f = _EftPlan(eft, 6, CPU)
        f.images_ptr = images.data_ptr()
        f.build_forward(6, 1024, 20, enc, 256)
        print(f"eft fwd linear_twin={int(linear_twin)}: {digest(f, arenas=(enc,), tensors=[('input_images', images)])}", flush=True)


if __name__ == "__main__":
    main()

"""Per-family A/B of the 4x4-level compile-time-geometry kernels (csrc/fused_gca4.h) and the (256, 16) row of k_gca_net0_t inside the replayed
B = 1 eval graph, in ONE process with interleaved rounds: the plan body is captured with every family on, with none (= the general kernels:
k_gca_pool, k_conv_fused, k_gca_pool_rc, k_gca_net0<16>), and with all but one, by setting the ops' keep bits; same buffers, same weights.
Prints the median eval time per mask over the rounds, the spread (max - min) between rounds of the SAME graph = the noise, and what each
family contributes (all-but-one minus all).   usage: gca4_ab.py [rounds]"""
import os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsefusion_amd import _lib
from sparsefusion_amd import unet as U
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
FAMILIES = ("k_gca_pool4_t (2 launches)", "k_conv4_1x1_t (1)", "k_gca_pool4_rc_t (2)", "k_gca_net0_t<256, 16> (2)")
dev = torch.device("cuda:0")
unet = U.Unet(channels=4, dim=256, dim_mults=(1, 2, 4, 4), num_resnet_blocks=(2, 2, 2, 2), layer_attns=(False, False, False, True),
              layer_cross_attns=(False,) * 4, cond_images_channels=256, attn_pool_text=False).to(dev)
x, cond = torch.randn(1, 4, 32, 32, device=dev), torch.randn(1, 256, 32, 32, device=dev)
ctx = unet.begin_sampling(cond, torch.linspace(-3, 3, 4, device=dev))
unet.eval_prepared(ctx, x, 0)
plan = ctx["plan"]
ops = [plan.body_array[k] for k in range(plan.n_body_ops)]
lib = _lib.lib()


def family(k):
    """Which family's kernel takes op k of the all-on plan (None: no new kernel); a res_conv || pooling pair is one family on both ops."""
    o = ops[k]
    paired = k > 0 and ops[k - 1].type == U.OP_FCONV and ops[k - 1].flags & 16
    if o.type == U.OP_GCA and o.flags == 1 and o.i[0] == 16 and o.i[2] == 16:
        return 2 if paired else 0
    if o.type == U.OP_FCONV and o.i[0] == 1 and o.i[1] == 4 and o.i[8] == 1 and o.i[12] == U.FNORM_NONE and o.i[3] + o.i[4] == 2048:
        return 2 if o.flags & 16 else 1
    if o.type == U.OP_GCA and o.flags == 2 and o.i[0] == 1 and o.i[1] == 256 and 8 < o.i[4] <= 16:
        return 3
    return None


def graph(mask):
    sub = (_lib.SfOp * len(ops))()
    for k, o in enumerate(ops):
        sub[k] = _lib.SfOp.from_buffer_copy(o)
        f = family(k)
        if f is not None and not (mask >> f) & 1:
            if o.type == U.OP_FCONV:
                sub[k].flags = o.flags | 256
            elif o.flags == 1:
                sub[k].i[8] = 1
            else:
                sub[k].i[5] = o.i[5] | 1
    n0 = [lib.sf_gca4_launches(j) for j in range(4)]
    run = lambda: _lib.check(lib.sf_plan_run(sub, len(ops), _lib.stream_ptr()), "sub-plan")
    run()
    torch.cuda.synchronize()
    took = [lib.sf_gca4_launches(j) - n0[j] for j in range(4)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        run()
    g.replay()
    torch.cuda.synchronize()
    return g, sub, took


ALL = 15
masks = [ALL, 0] + [ALL ^ (1 << j) for j in range(4)]
graphs = {m: graph(m) for m in masks}
times = {m: [] for m in masks}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(ROUNDS + 1):
    for m in masks:
        e0.record()
        for _ in range(50):
            graphs[m][0].replay()
        e1.record()
        torch.cuda.synchronize()
        if r:                                            # round 0 warms every graph
            times[m].append(e0.elapsed_time(e1) / 50 * 1e3)
med = {m: statistics.median(v) for m, v in times.items()}
for m in masks:
    name = "all on" if m == ALL else "all off" if m == 0 else "without " + FAMILIES[(ALL ^ m).bit_length() - 1]
    print(f"mask {m:2d} {name:42s} launches {graphs[m][2]}  median {med[m]:7.1f} us  min {min(times[m]):7.1f}  spread {max(times[m]) - min(times[m]):4.1f}  "
          f"vs all on {med[m] - med[ALL]:+5.1f} us")

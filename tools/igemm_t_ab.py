"""Per-variant A/B of k_conv_igemm_t inside the replayed B = 1 eval graph, in ONE process with interleaved rounds: the plan body is captured
with op flag 512 (csrc/conv_igemm_t.h) kept on every marked op, on none, and on all but one; same buffers, same weights.  Prints the
median eval time per mask over the rounds, the spread (max - min) between rounds of the SAME graph = the noise, and what each variant
contributes (all-but-one minus all).   usage: igemm_t_ab.py [rounds]"""
import os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsefusion_amd import _lib
from sparsefusion_amd import unet as U
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
unet = U.Unet(channels=4, dim=256, dim_mults=(1, 2, 4, 4), num_resnet_blocks=(2, 2, 2, 2), layer_attns=(False, False, False, True),
              layer_cross_attns=(False,) * 4, cond_images_channels=256, attn_pool_text=False).to(dev)
x, cond = torch.randn(1, 4, 32, 32, device=dev), torch.randn(1, 256, 32, 32, device=dev)
ctx = unet.begin_sampling(cond, torch.linspace(-3, 3, 4, device=dev))
unet.eval_prepared(ctx, x, 0)
plan = ctx["plan"]
ops = [plan.body_array[k] for k in range(plan.n_body_ops)]
lib = _lib.lib()


def row(o):
    key = (o.i[1].bit_length() - 1, o.i[3], o.i[6], o.i[9], o.i[11], o.i[12], 1 if o.flags & 16 else 0, o.i[14] // 16, o.i[14] % 16, o.i[13],
           o.flags & 1, 1 if o.flags & 2 else 0)
    return U.IGEMM_T_VARIANTS.index(key)


def graph(mask):
    sub = (_lib.SfOp * len(ops))()
    for k, o in enumerate(ops):
        sub[k] = _lib.SfOp.from_buffer_copy(o)
        if o.type == U.OP_CONV and o.flags & 512 and not (mask >> row(o)) & 1:
            sub[k].flags = o.flags & ~512
    run = lambda: _lib.check(lib.sf_plan_run(sub, len(ops), _lib.stream_ptr()), "sub-plan")
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        run()
    g.replay()
    torch.cuda.synchronize()
    return g, sub


n = len(U.IGEMM_T_VARIANTS)
ALL = (1 << n) - 1
masks = [ALL, 0] + [ALL ^ (1 << j) for j in range(n)]
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
    name = "all on" if m == ALL else "all off" if m == 0 else "without row %d %s" % ((ALL ^ m).bit_length() - 1, U.IGEMM_T_VARIANTS[(ALL ^ m).bit_length() - 1])
    print(f"mask {m:3d} {name:70s} median {med[m]:7.1f} us  min {min(times[m]):7.1f}  spread {max(times[m]) - min(times[m]):4.1f}  "
          f"vs all on {med[m] - med[ALL]:+5.1f} us")

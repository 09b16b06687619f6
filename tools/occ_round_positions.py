"""Sample positions of the reference's evaluation ROUND LOOP against ONE uninterrupted march, on the C oracle (no GPU needed).
renderer_df.py:523-556 marches n_step samples per round and restarts each round from rays_t = near + the gaps composite_rays summed;
the one-launch kernels (sf_ngp_render_occ_eval, sf_ngp_render_occ_eval_shaded) and the one-round route of the tests keep the
marcher's own t.  The two t differ by float32 rounding, so a few rays get sample positions an ulp or two apart (why
the image of tools/occ_eval_time.py's round loop (c) differs from the one-launch render (a) on the dense ball scene).  All sigmas are
zero here, so no ray ends by T_thresh and the comparison is of positions alone.
usage: occ_round_positions.py [--side 64] [--max-steps 256]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from oracle import ngp_native, ngp_ref
from occ_common import BOUND, CASCADE, H, ball_bitfield
ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=64)
ap.add_argument("--max-steps", type=int, default=256)                   # get_default_torch_ngp_opt().max_steps, what the timing tool passes
args = ap.parse_args()
S = args.max_steps
_, bits, _ = ball_bitfield()                                            # radius 1.3 at (0.2, -0.1, 0.3): occ_eval_time.py --scene ball
o, d = ngp_ref.circle_rays(args.side, view=3)
o, d = o.contiguous(), d.contiguous()
N = o.shape[0]
aabb = torch.tensor([-BOUND, -BOUND, -BOUND, BOUND, BOUND, BOUND])
nears, fars = torch.empty(N), torch.empty(N)
ngp_native.near_far_from_aabb(o, d, aabb, N, 0.2, nears, fars)


def march(n_alive, n_step, alive, rays_t):
    x, dr, dl = torch.zeros(n_alive * n_step, 3), torch.zeros(n_alive * n_step, 3), torch.zeros(n_alive * n_step, 2)
    ngp_native.march_rays(n_alive, n_step, alive, rays_t, o, d, BOUND, 0.0, S, CASCADE, H, bits, nears, fars, x, dr, dl, torch.zeros(N))
    return x.view(n_alive, n_step, 3), dl.view(n_alive, n_step, 2)


one_x, one_dl = march(N, S, torch.arange(N, dtype=torch.int32), nears.clone())
one_n = (one_dl[..., 0] != 0).sum(1)
loop_x, loop_n = torch.zeros(N, S, 3), torch.zeros(N, dtype=torch.long)
alive, rays_t, step = torch.arange(N, dtype=torch.int32), nears.clone(), 0
ws, depth, image = torch.zeros(N), torch.zeros(N), torch.zeros(N, 3)
while step < S and alive.numel() > 0:
    n_alive = alive.numel()
    n_step = max(min(N // n_alive, 8), 1)
    x, dl = march(n_alive, n_step, alive, rays_t)
    for k, r in enumerate(alive.tolist()):
        m = int((dl[k, :, 0] != 0).sum())
        m = min(m, S - int(loop_n[r]))
        loop_x[r, loop_n[r]:loop_n[r] + m] = x[k, :m]
        loop_n[r] += m
    ngp_native.composite_rays(n_alive, n_step, 1e-4, alive, rays_t, torch.zeros(n_alive * n_step), torch.zeros(n_alive * n_step, 3),
                              dl.reshape(-1, 2).contiguous(), ws, depth, image)
    alive = alive[alive >= 0].contiguous()
    step += n_step
hit = one_n > 0
common = torch.minimum(one_n, loop_n)
diff = torch.zeros(N)
for r in torch.nonzero(hit).flatten().tolist():
    m = int(common[r])
    if m:
        diff[r] = (one_x[r, :m] - loop_x[r, :m]).abs().max()
print(f"{args.side}x{args.side} rays, max_steps {S}: {int(hit.sum())} rays hit the ball ({int(one_n.sum())} samples); rays whose sample "
      f"positions differ between the round loop and one march: {int((diff > 0).sum())}, by at most {float(diff.max()):.2e}; rays whose "
      f"sample count differs: {int((one_n != loop_n).sum())}")

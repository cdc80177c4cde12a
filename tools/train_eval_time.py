#!/usr/bin/env python
"""Time of one test render of the student's training loop (efficient-nerf_amd/train.py eval_test_split) at the README size: the 25
test views `configs/lego_noview.txt --testskip 8` selects, 400 x 400, W256D88, from the weights in the trainer's buffer at the README
batch (98,304 rays per chunk), with the metrics and without writing the PNGs; beside it one training step on the same trainer, so
that the share `--i_testset 2000` costs can be read off.  HIP events after warm-up.  Synthetic poses and ground truth: the time
does not depend on them.  Writes profiles/train_eval_time.txt.

    python tools/train_eval_time.py [--views 25] [--size 400] [--rays 98304] [--repeat 3] [--out profiles/train_eval_time.txt]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd.frontend import pose_spherical  # noqa: E402
from efficient_nerf_amd.train import R2LTrainer, eval_test_split, init_state_dict  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=25)
    ap.add_argument('--size', type=int, default=400)
    ap.add_argument('--rays', type=int, default=98304)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--i_testset', type=int, default=2000)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'train_eval_time.txt'))
    a = ap.parse_args()
    n, H = a.rays, a.size
    tr = R2LTrainer(netdepth=88, netwidth=256, use_residual=True, trial=dict(body_arch='resmlp'), max_rays=n)
    tr.load_state_dict(init_state_dict(tr.plan, seed=0))
    g = torch.Generator().manual_seed(0)
    poses = torch.stack([pose_spherical(t, -30., 4.) for t in np.linspace(-180, 180, a.views + 1)[:-1]], 0)
    focal = .5 * H / np.tan(.5 * 0.6911112070083618)
    test = (poses, (H, H, focal), torch.rand(a.views, H, H, 3, generator=g).cuda())
    ro = (torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)).cuda()
    rd = torch.nn.functional.normalize(-ro.cpu() + 0.8 * torch.randn(n, 3, generator=g), dim=-1).cuda()
    tgt = torch.rand(n, 3, generator=g).cuda()
    step_ms = timed(lambda: tr.step(ro, rd, tgt, 1e-4, 1.), 5, 2)
    eval_ms = timed(lambda: eval_test_split(tr, test), a.repeat, 1)
    render_ms = timed(lambda: [tr.render(p, H, H, focal) for p in poses], a.repeat, 1)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        eval_test_split(tr, test, savedir=d)
        torch.cuda.synchronize()
        png_s = time.time() - t0 - eval_ms * 1e-3
    rays = a.views * H * H
    every = a.i_testset * step_ms
    lines = [f'eval_test_split on R2LTrainer, W256D88, {a.views} views of {H} x {H} = {rays} rays in chunks of {n} (the README batch); HIP events, '
             f'{a.repeat} runs after 1 warm-up run',
             f'test render with PSNR / PSNRv2 / SSIM: {eval_ms:.1f} ms = {rays / eval_ms * 1e3:.3e} rays/s (the renders alone: {render_ms:.1f} ms = '
             f'{rays / render_ms * 1e3:.3e} rays/s = {tr.flops_per_ray * rays / (render_ms * 1e-3) / 1e12:.1f} TFLOP/s fp32)',
             f'writing the {a.views} PNGs on the host: {png_s:.2f} s more (host clock)',
             f'one training step on the same trainer, {n} rays: {step_ms:.2f} ms; --i_testset {a.i_testset}: {every / 1e3:.1f} s of steps between two test '
             f'renders, of which a render is {eval_ms / every * 100:.2f} % ({(eval_ms + png_s * 1e3) / every * 100:.2f} % with the PNGs)']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()

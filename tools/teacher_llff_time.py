#!/usr/bin/env python
"""Time of one LLFF teacher step at configs/fern.txt (1,024 rays, 64 + 64 samples, and 64 + 128 as configs/lego.txt has them, two
8 x 256 networks with view directions, raw_noise_std 1, NDC) on a synthetic 17 x 378 x 504 byte stack (fern at --factor 8), of nerf_train_batch_rays alone, and of
the chain of existing launches it replaces on the same window: r2l_rays_from_images, three strided slice copies, torch's norm and
division, nerf_ndc_rays.  HIP events; every figure is the median of 5 windows with the smallest and the largest beside it.  Writes
profiles/teacher_llff_step_time.txt.

    python tools/teacher_llff_time.py [--rays 1024] [--N_importance 64,128] [--steps 10] [--calls 200] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import teacher as T  # noqa: E402
from efficient_nerf_amd import train_teacher as TT  # noqa: E402
from efficient_nerf_amd._lib import check, current_stream, dptr, lib  # noqa: E402

WINDOWS = 5


def windows(fn, calls, warmup):
    """ms per call: (median, smallest, largest) of WINDOWS windows of `calls` calls"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return float(np.median(out)), min(out), max(out)


def fmt(t, unit='ms'):
    k = 1e3 if unit == 'us' else 1.
    return f'{t[0] * k:.2f} {unit} ({t[1] * k:.2f} .. {t[2] * k:.2f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--N_samples', type=int, default=64)
    ap.add_argument('--N_importance', type=str, default='64,128')
    ap.add_argument('--steps', type=int, default=10, help='steps per window')
    ap.add_argument('--calls', type=int, default=200, help='ray launches per window')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'teacher_llff_step_time.txt'))
    a = ap.parse_args()
    n_img, H, W, focal, n = 17, 378, 504, 407.5657, a.rays
    g = torch.Generator().manual_seed(0)
    image_bytes = torch.randint(0, 256, (n_img, H, W, 3), generator=g, dtype=torch.uint8)
    poses = torch.eye(3, 4).repeat(n_img, 1, 1) + 0.05 * torch.randn(n_img, 3, 4, generator=g)
    np.random.seed(0)
    torch.manual_seed(0)
    rb = TT.RayBatches(image_bytes, poses, focal, n, True, log=lambda *_: None)
    t_steps = {}
    for n_imp in (int(v) for v in a.N_importance.split(',')):
        tr = TT.NeRFTrainer(0., 1., N_samples=a.N_samples, N_importance=n_imp, max_rays=n)
        tr.load_state_dicts(*tr.init_state_dicts(seed=0))

        def step():
            ro, rd, vd, tgt = rb.next()
            tr.step(ro, rd, tgt, 1e-4, perturb=1., raw_noise_std=1., viewdirs=vd)

        t_steps[n_imp] = windows(step, a.steps, a.warmup)
        del tr
        torch.cuda.empty_cache()
    t_new = windows(lambda: rb._launch(0, n), a.calls, a.warmup)
    order = rb._order[:n]
    L = lib()

    def chain():
        rows9 = torch.empty((n, 9), dtype=torch.float32, device=rb.device)
        check(L.r2l_rays_from_images(rb._bytes.data_ptr(), n_img, H, W, 3, dptr(rb._poses), focal, 0, order.data_ptr(), n, dptr(rows9),
                                     current_stream()))
        ro, rd, tgt = rows9[:, 0:3].contiguous(), rows9[:, 3:6].contiguous(), rows9[:, 6:9].contiguous()
        vd = rd / torch.norm(rd, dim=-1, keepdim=True)
        no, nd = T.ndc_rays(H, W, focal, 1., ro, rd)
        return no, nd, vd, tgt

    new, old = rb._launch(0, n), chain()
    same = all(torch.equal(x, y) for x, y in zip((new[0], new[1], new[3]), (old[0], old[1], old[3])))
    vgap = float((new[2] - old[2]).abs().max())
    t_old = windows(chain, a.calls, a.warmup)
    bank = rb.n * 36
    lines = [f'LLFF teacher step at configs/fern.txt: {n} rays, two 8 x 256 networks with view '
             f'directions, raw_noise_std 1, NDC; synthetic bytes [{n_img}, {H}, {W}, 3] = {rb.n} training rays.  HIP events, medians of '
             f'{WINDOWS} windows (smallest .. largest).',
             *[f'step (RayBatches.next + NeRFTrainer.step) at {a.N_samples} + {k} samples, {a.steps} steps per window: {fmt(t)}; --N_iters 200000 '
               f'at this step time: {200000 * t[0] / 3.6e6:.2f} h (one box, one run)' for k, t in t_steps.items()],
             f'nerf_train_batch_rays alone (one launch, four [n, 3] outputs), {a.calls} calls per window: {fmt(t_new, "us")}',
             f'the chain it replaces (r2l_rays_from_images, three slice copies, norm, division, nerf_ndc_rays), same window: {fmt(t_old, "us")}',
             f'  rays_o / rays_d / target of the two bit-equal: {same}; largest |viewdirs| difference {vgap:.1e}',
             f'resident on the device: bytes {image_bytes.numel() / 1e6:.1f} MB + permutation {rb.n * 8 / 1e6:.1f} MB; the reference\'s '
             f'bank of [n, 3, 3] float32 rows would be {bank / 1e6:.1f} MB']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

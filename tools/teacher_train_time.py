#!/usr/bin/env python
"""Time of one training step of the NeRF teacher at the README batch (configs/lego.txt: 1,024 rays, 64 + 128 samples, two 8 x 256
networks with view directions; --N_importance 192 for the issue's 64 + 192 estimate) on NeRFTrainer, its split into forward / g_x /
g_W / scans / element-wise, and the same step under PyTorch-ROCm autograd of the oracle's functions on the same box.  HIP events
after warm-up.  Writes profiles/teacher_train_step_time.txt.

    python tools/teacher_train_time.py [--rays 1024] [--N_importance 128] [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import teacher as T  # noqa: E402
from efficient_nerf_amd import train_teacher as TT  # noqa: E402

PEAK_TFLOPS = 157.3      # fp32 MFMA: 256 FLOP/clk/CU x 256 CUs x 2.4 GHz (csrc/r2l_generic.hip's header)
STAGES = {'_linear': 'forward', '_grad_input': 'g_x', '_grad_weight': 'g_W', '_scan_forward': 'scans', '_scan_backward': 'scans',
          '_act_backward': 'element-wise', '_embed': 'element-wise', 'adam': 'element-wise'}


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


class StageEvents:
    """an event pair around every launch method of a trainer (and the sampling functions of the teacher module), summed per stage"""

    def __init__(self):
        self.pairs = {}

    def wrap(self, obj, name, stage):
        fn = getattr(obj, name)

        def timed_call(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            self.pairs.setdefault(stage, []).append((s, e))
            return out
        setattr(obj, name, timed_call)
        return fn

    def totals(self):
        torch.cuda.synchronize()
        return {k: sum(s.elapsed_time(e) for s, e in v) for k, v in self.pairs.items()}


def torch_step_fn(O, tr, sds, ro, rd, tgt, t_rand, u):
    """render_rays (main.py:624-756) with perturb = 1 + both losses + Adam under autograd, from the oracle's functions"""
    prm = [{k: v.detach().cuda().clone().requires_grad_(True) for k, v in sd.items()} for sd in sds]
    opt = torch.optim.Adam([p for d in prm for p in d.values()], lr=1e-4, betas=(0.9, 0.999))
    net = dict(multires=tr.multires, multires_views=tr.multires_views, i_embed=0, use_viewdirs=True)
    z_coarse = tr.z_coarse.cuda()
    n = ro.shape[0]

    def step():
        vd = rd / torch.norm(rd, dim=-1, keepdim=True)
        z0 = O.perturb_z_vals(z_coarse.expand(n, -1), t_rand=t_rand)
        raw0 = O.run_network_generic(prm[0], ro[:, None, :] + rd[:, None, :] * z0[:, :, None], vd, **net)
        rgb0, _, _, w0, _ = O.raw2outputs(raw0, z0, rd, white_bkgd=tr.white_bkgd)
        z_s = O.sample_pdf(.5 * (z0[:, 1:] + z0[:, :-1]), w0[:, 1:-1], tr.N_importance, det=False, u=u).detach()
        z1 = O.merge_z(z0, z_s)
        raw1 = O.run_network_generic(prm[1], ro[:, None, :] + rd[:, None, :] * z1[:, :, None], vd, **net)
        rgb = O.raw2outputs(raw1, z1, rd, white_bkgd=tr.white_bkgd)[0]
        loss = ((rgb0 - tgt) ** 2).mean() + ((rgb - tgt) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--N_samples', type=int, default=64)
    ap.add_argument('--N_importance', type=int, default=128)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no_torch', action='store_true')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'teacher_train_step_time.txt'))
    a = ap.parse_args()
    n = a.rays
    tr = TT.NeRFTrainer(N_samples=a.N_samples, N_importance=a.N_importance, white_bkgd=True, max_rays=n)
    sds = tr.init_state_dicts(seed=0)
    tr.load_state_dicts(*sds)
    g = torch.Generator().manual_seed(0)
    o = torch.randn(n, 3, generator=g)
    o = 4. * o / o.norm(dim=-1, keepdim=True)
    ro, rd = o.cuda(), (-o / 4. + 0.15 * torch.randn(n, 3, generator=g)).cuda()
    tgt = torch.rand(n, 3, generator=g).cuda()
    t_rand, u = torch.rand(n, a.N_samples, generator=g).cuda(), torch.rand(n, a.N_importance, generator=g).cuda()
    step = lambda: tr.step(ro, rd, tgt, 1e-4, perturb=1., t_rand=t_rand, u=u)
    step_ms = timed(step, a.steps, a.warmup)
    # the stages: the same steps again with an event pair around every launch method
    ev = StageEvents()
    for name, stage in STAGES.items():
        ev.wrap(tr, name, stage)
    keep = {name: ev.wrap(T, name, 'scans') for name in ('sample_pdf', 'merge_sorted')}
    for _ in range(a.steps):
        step()
    ms = {k: v / a.steps for k, v in ev.totals().items()}
    for name, fn in keep.items():
        setattr(T, name, fn)
    fl = tr.flops_per_ray
    first = sum(2 * net.S * net.layers['pts_linears.0'][0] * net.W for net in tr.nets)        # no g_x for the two first layers
    part_fl = {'forward': fl, 'g_W': fl, 'g_x': fl - first}
    rate = lambda k, t: part_fl[k] * n / (t * 1e-3) / 1e12
    total = (3 * fl - first) * n
    lines = [f'NeRFTrainer.step, two 8 x 256 networks with view directions, {n} rays per step, {a.N_samples} samples in the coarse pass and '
             f'{a.N_samples + a.N_importance} in the fine pass ({tr.n_param} parameters, saved activations {tr.activation_bytes(n) / 2 ** 30:.2f} GiB), HIP events over {a.steps} '
             f'steps after {a.warmup} warm-up steps',
             f'step: {step_ms:.2f} ms = {total / 1e12:.3f} TFLOP (forward + g_x + g_W of every layer) at {total / (step_ms * 1e-3) / 1e12:.1f} '
             f'TFLOP/s ({total / (step_ms * 1e-3) / 1e12 / PEAK_TFLOPS:.2f} of the fp32 MFMA peak, {PEAK_TFLOPS} TFLOP/s)']
    for k in ('forward', 'g_x', 'g_W', 'scans', 'element-wise'):
        t = ms.get(k, 0.)
        extra = f' = {rate(k, t):.1f} TFLOP/s ({rate(k, t) / PEAK_TFLOPS:.2f} of the peak)' if k in part_fl and t > 0 else ''
        lines.append(f'  {k}: {t:.2f} ms{extra}')
    lines.append(f'  sum of the stages (event pairs around single launches): {sum(ms.values()):.2f} ms; scans = raw2outputs forward and '
                 f'backward, sample_pdf, merge; element-wise = relu backward, embedding, Adam')
    if not a.no_torch:
        from oracle import r2l_oracle as O
        t_ms = timed(torch_step_fn(O, tr, sds, ro, rd, tgt, t_rand, u), a.steps, a.warmup)
        lines.append(f'the same step under PyTorch-ROCm autograd (fp32, same draws): {t_ms:.2f} ms ({t_ms / step_ms:.2f} x)')
    lines.append(f'--N_iters 200000 at this step time: {200000 * step_ms / 3.6e6:.2f} h (one box, one run)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

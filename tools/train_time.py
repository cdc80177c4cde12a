#!/usr/bin/env python
"""Time of one training step of the R2L student at the README batch (98,304 rays = 20 shards + 20 % hard rays, W256D88) on
R2LTrainer, its split into forward / g_x / g_W / element-wise / Adam, and the same step under PyTorch-ROCm autograd on the same
box.  HIP events after warm-up.  Writes profiles/train_step_time.txt.

    python tools/train_time.py [--rays 98304] [--steps 5] [--warmup 2] [--out profiles/train_step_time.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd.generic import _act_code  # noqa: E402
from efficient_nerf_amd.train import R2LTrainer, init_state_dict  # noqa: E402

PEAK_TFLOPS = 157.3      # fp32 MFMA: 256 FLOP/clk/CU x 256 CUs x 2.4 GHz (csrc/r2l_generic.hip's header)


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
    ap.add_argument('--rays', type=int, default=98304)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no_torch', action='store_true')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'train_step_time.txt'))
    a = ap.parse_args()
    n = a.rays
    trial = dict(body_arch='resmlp')
    tr = R2LTrainer(netdepth=88, netwidth=256, use_residual=True, trial=trial, max_rays=n)
    sd = init_state_dict(tr.plan, seed=0)
    tr.load_state_dict(sd)
    g = torch.Generator().manual_seed(0)
    ro = (torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)).cuda()
    rd = torch.nn.functional.normalize(-ro.cpu() + 0.8 * torch.randn(n, 3, generator=g), dim=-1).cuda()
    tgt = torch.rand(n, 3, generator=g).cuda()
    t_rand = torch.rand(n, 16, generator=g).cuda()
    step_ms = timed(lambda: tr.step(ro, rd, tgt, 1e-4, 1., t_rand), a.steps, a.warmup)
    # the parts, each over all layers, on the buffers the step left
    acts = [x[:n] for x in tr._acts]
    R, Y, Z, P = (b[:n] for b in tr._gbuf)
    emb = tr._emb[:n]
    body = range(1, len(tr.plan) - 1)
    parts = {
        'sample + embed': lambda: tr.embed(ro, rd, 1., t_rand),
        'forward': lambda: tr.forward(emb, n),
        'g_x': lambda: [tr._grad_input(p['key'], Z[:, :p['out_dim']], Y[:, :p['in_dim']], False) for p in tr.plan[1:]],
        'g_W': lambda: [tr._grad_weight(p['key'], Z[:, :p['out_dim']], emb if i == 0 else acts[i - 1]) for i, p in enumerate(tr.plan)],
        'element-wise': lambda: [tr._act_backward(tr.plan[i]['key'], R[:, :tr.plan[i]['out_dim']], acts[i], Z[:, :tr.plan[i]['out_dim']],
                                                  _act_code(tr.plan[i]['act']),
                                                  g_res=R[:, :tr.plan[i]['out_dim']] if tr.plan[i].get('block_out') else None)
                                 for i in [0] + list(body)],
        'Adam': lambda: tr.adam(0.0),
    }
    ms = {k: timed(fn, a.steps, 1) for k, fn in parts.items()}
    fl = tr.flops_per_ray
    part_fl = {'forward': fl, 'g_W': fl, 'g_x': fl - 2 * tr.plan[0]['in_dim'] * tr.plan[0]['out_dim']}      # no g_x for the head layer
    gemm = lambda k, t: part_fl[k] * n / (t * 1e-3) / 1e12
    lines = [f'R2LTrainer.step, W256D88, {n} rays per step ({len(tr.plan)} layers, {tr.n_param} parameters, saved activations '
             f'{tr.activation_bytes(n) / 2 ** 30:.2f} GiB), HIP events over {a.steps} steps after {a.warmup} warm-up steps',
             f'step: {step_ms:.2f} ms = {n / step_ms * 1e3:.3e} rays/s = {3 * fl * n / (step_ms * 1e-3) / 1e12:.1f} TFLOP/s at 3 x flops_per_ray '
             f'({3 * fl * n / (step_ms * 1e-3) / 1e12 / PEAK_TFLOPS:.2f} of the fp32 MFMA peak, {PEAK_TFLOPS} TFLOP/s)']
    for k, t in ms.items():
        extra = f' = {gemm(k, t):.1f} TFLOP/s ({gemm(k, t) / PEAK_TFLOPS:.2f} of the peak)' if k in part_fl else ''
        lines.append(f'  {k}: {t:.2f} ms{extra}')
    lines.append(f'  sum of the parts: {sum(ms.values()):.2f} ms')
    lines.append(f'  rate against the forward kernel on this run: g_x {gemm("g_x", ms["g_x"]) / gemm("forward", ms["forward"]):.2f}, '
                 f'g_W {gemm("g_W", ms["g_W"]) / gemm("forward", ms["forward"]):.2f}')
    if not a.no_torch:
        from oracle import r2l_oracle as O
        prm = {k: v.detach().cuda().clone().requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.Adam(list(prm.values()), lr=1e-4, betas=(0.9, 0.999))
        emb_c = emb.clone()

        def torch_step():
            loss = ((O.r2l_forward(prm, emb_c) - tgt) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
        t_ms = timed(torch_step, a.steps, a.warmup)
        lines.append(f'the same step under PyTorch-ROCm autograd (fp32, embedding given): {t_ms:.2f} ms ({t_ms / step_ms:.2f} x)')
    lines.append(f'--N_iters 1200000 at this step time: {1200000 * step_ms / 3.6e6:.1f} h (one box, one run)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()

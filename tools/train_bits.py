#!/usr/bin/env python
"""sha256 of what three training steps leave behind, for both trainers, to compare two checkouts bit for bit on one build of the
library: the flat parameter, gradient and moment buffers, the three losses and the err / loss_rgb returned.  Fixed seeds, given
draws (t_rand, u, noise), three learning rates; only public trainer methods, so the same file runs against any checkout that has
both trainers.  The cases are the SMALL lists of tests/test_train_gpu.py and tests/test_train_teacher_gpu.py at 300 rays, W256D88 at
2,048 rays and the 8 x 256 pair at 512 rays.

    python tools/train_bits.py [--tree CHECKOUT] > bits.txt      # R2L_LIB_PATH=... to share one library between two checkouts
"""
import argparse
import hashlib
import os
import sys

import torch

LRS = (5e-4, 1e-3, 2e-4)

STUDENT_SMALL = [
    # netdepth, netwidth, layerwise_netwidths, act, use_residual, trial
    (8, 96, '', 'relu', True, dict(body_arch='resmlp', n_block=2, n_learnable=3, res_scale=0.5, inact='lrelu', outact='none')),
    (6, 64, '', 'lrelu', False, dict(body_arch='resmlp', n_learnable=2, res_scale=1.0, inact='relu', outact='relu')),
    (6, 48, '', 'relu', True, None),
    (6, 64, '64,48,48,32,64', 'lrelu', True, None),
    (4, 32, '', 'relu', True, dict(body_arch='resmlp', n_block=1, n_learnable=2, res_scale=0.5, inact='relu', outact='lrelu')),
    (5, 40, '', 'relu', False, dict(body_arch='resmlp', n_block=2, n_learnable=1, res_scale=1.0, inact='relu', outact='none')),
]
TEACHER_BASE = dict(N_samples=12, N_importance=10, multires=4, multires_views=2, i_embed=0, netdepth=4, netwidth=64, netdepth_fine=4,
                    netwidth_fine=64, use_viewdirs=True, white_bkgd=True, lindisp=False)
TEACHER_SMALL = [
    ('D4 W128 coarse, D6 W64 fine', dict(netdepth=4, netwidth=128, netdepth_fine=6, netwidth_fine=64), 0.),
    ('no view directions (output_ch 5)', dict(use_viewdirs=False, netdepth=6, netdepth_fine=6), 0.),
    ('N_importance 0', dict(N_importance=0, netdepth=6), 0.),
    ('N_importance 0, no view directions (output_ch 4)', dict(N_importance=0, use_viewdirs=False), 0.),
    ('black background', dict(white_bkgd=False), 0.),
    ('raw_noise_std 1', dict(), 1.),
    ('i_embed -1', dict(i_embed=-1), 0.),
    ('lindisp', dict(lindisp=True, netdepth=8, netdepth_fine=7), 0.),
]


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().to('cpu', torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


def report(label, tr, losses, seconds, dicts):
    """dicts: callables returning the parameter / gradient dicts of every network (None for a missing one)"""
    flat = lambda ds: [v for d in ds if d is not None for v in d.values()]
    osd = tr.optimizer_state_dict()['state']
    params, grads = dicts
    print(f'{label}: param {sha(flat(params()))} grad {sha(flat(grads()))} exp_avg {sha(osd[k]["exp_avg"] for k in sorted(osd))} '
          f'exp_avg_sq {sha(osd[k]["exp_avg_sq"] for k in sorted(osd))} losses {sha(losses)} second {sha(seconds)}', flush=True)


def student_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)
    d = -o + 0.8 * torch.randn(n, 3, generator=g)
    return o.cuda(), (d / d.norm(dim=-1, keepdim=True)).cuda()


def student_case(label, tr, sd, n, seed):
    tr.load_state_dict(sd)
    ro, rd = student_rays(n, seed)
    g = torch.Generator().manual_seed(200 + seed)
    losses, seconds = [], []
    for lr in LRS:
        target, t_rand = torch.rand(n, 3, generator=g).cuda(), torch.rand(n, tr.n_sample, generator=g).cuda()
        loss, err = tr.step(ro, rd, target, lr, 1., t_rand)
        losses.append(loss.clone()), seconds.append(err.clone())
    report(label, tr, losses, seconds, (lambda: [tr.state_dict()], lambda: [tr.grads()]))


def teacher_case(label, tr, sds, n, seed, raw_noise_std):
    tr.load_state_dicts(*sds)
    g = torch.Generator().manual_seed(1000 + seed)
    o = torch.randn(n, 3, generator=g)
    o = 4. * o / o.norm(dim=-1, keepdim=True)
    ro, rd = o.cuda(), (-o / 4. + 0.15 * torch.randn(n, 3, generator=g)).cuda()
    losses, seconds = [], []
    for lr in LRS:
        target, t_rand = torch.rand(n, 3, generator=g).cuda(), torch.rand(n, tr.N_samples, generator=g).cuda()
        u = torch.rand(n, tr.N_importance, generator=g).cuda() if tr.N_importance > 0 else None
        noise = tuple(raw_noise_std * torch.randn(n, net.S, generator=g).cuda() for net in tr.nets) if raw_noise_std > 0 else None
        loss, loss_rgb = tr.step(ro, rd, target, lr, perturb=1., t_rand=t_rand, u=u, noise=noise)
        losses.append(loss.clone()), seconds.append(loss_rgb.clone())
    report(label, tr, losses, seconds, (tr.state_dicts, tr.grads))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the checkout whose package runs')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import _pkg
    _pkg.load()
    from efficient_nerf_amd.train import R2LTrainer
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    for case, (D, W, lw, act, use_res, trial) in enumerate(STUDENT_SMALL):
        tr = R2LTrainer(n_sample=4, L=3, netdepth=D, netwidth=W, layerwise_netwidths=lw, act=act, use_residual=use_res, trial=trial,
                        max_rays=300)
        student_case(f'student small {case}', tr, O.make_v3_2_state(case, D, W, tr.input_dim, lw, act, trial), 300, 50 + case)
    tr = R2LTrainer(netdepth=88, netwidth=256, use_residual=True, trial=dict(body_arch='resmlp'), max_rays=2048)
    student_case('student W256D88', tr, O.make_r2l_state(0), 2048, 0)
    nerf_states = lambda tr, seed: [O.make_nerf_state(seed * 2 + k, net.D, net.W, tr.input_ch, tr.input_ch_views, tr.output_ch, (4,),
                                                      tr.use_viewdirs) for k, net in enumerate(tr.nets)]
    for case, (label, kw, std) in enumerate(TEACHER_SMALL):
        tr = NeRFTrainer(max_rays=300, **dict(TEACHER_BASE, **kw))
        teacher_case(f'teacher small {case} ({label})', tr, nerf_states(tr, 10 + case), 300, 10 + case, std)
    tr = NeRFTrainer(N_samples=64, N_importance=128, white_bkgd=True, max_rays=512)
    teacher_case('teacher 8 x 256 pair', tr, nerf_states(tr, 0), 512, 0, 0.)


if __name__ == '__main__':
    main()

"""GPU: training of the NeRF teacher in the library's fp32 kernels (csrc/nerf_train.hip, efficient-nerf_amd/train_teacher.py).

Yardstick: float64 torch autograd of oracle/r2l_oracle.py's functions (raw2outputs, nerf_forward).  Scale: the gap torch's own
fp32 autograd of the same functions keeps from float64, measured in the same test; the HIP gap may be 4 x that (another fp32
summation order, nothing more).  Gaps are relative L2, global and worst per tensor, printed before they are asserted."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope='module')
def L(pkg, built_lib):
    from efficient_nerf_amd import _lib
    return _lib.lib()


def _rel(got, ref):
    den = float(ref.double().norm())
    num = float((got.double() - ref.double()).norm())
    return num / den if den > 0 else (0. if num == 0 else float('inf'))


# ---- 1. the scan's backward pass alone ---------------------------------------------------------------------------------------
def _scan_case(n, S, kind, seed):
    """raw [n,S,4], per-ray sorted z [n,S], rays_d [n,3], g_rgb_map [n,3].  kind: 'thin' (densities N(0.6, 2): no sample
    saturates, torch's own fp32 band is tight), 'mixed' (densities N(0, 1) ... N(0, 300): empty
    stretches and sigma up to several hundred), 'empty' (no sample with a positive density), 'saturated' (an interior stretch with
    sigma = 300 ... 3000: alpha = 1 in fp32)"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, S, 4, generator=g)
    scale = 10 ** (2.5 * torch.rand(n, 1, generator=g))
    raw[..., 3] = raw[..., 3] * scale + 0.3 * scale
    if kind == 'thin':
        raw[..., 3] = 2. * torch.randn(n, S, generator=g) + 0.6
    if kind == 'empty':
        raw[..., 3] = -raw[..., 3].abs() - 0.5
    if kind == 'saturated' and S >= 3:
        a = S // 3
        raw[:, a:a + max(1, S // 8), 3] = 300. * (1 + 9 * torch.rand(n, 1, generator=g))
    z = torch.sort(2. + 4. * torch.rand(n, S, generator=g), -1)[0]
    rd = torch.randn(n, 3, generator=g)
    g_rgb = torch.randn(n, 3, generator=g)
    return raw, z, rd, g_rgb


def _raw2outputs_one_sample(raw, rd, white, noise):
    """O.raw2outputs' expressions for S = 1 with dists = [1e10] written out.  The oracle (and the reference) build that column as
    Tensor([1e10]).expand(dists[..., :1].shape), which is empty when there is no interval: at S = 1 they composite nothing.  The
    library's forward scan (nerf_raw2outputs) keeps the column as the formula cat(z[1:] - z[:-1], 1e10) states it, and the backward
    pass is the gradient of that forward: test_scan_backward_one_sample_matches_the_forward_kernel ties the two together."""
    dists = torch.full_like(raw[..., 3], 1e10) * torch.norm(rd[..., None, :], dim=-1)
    alpha = 1. - torch.exp(-torch.relu(raw[..., 3] + (0. if noise is None else noise)) * dists)
    rgb_map = torch.sum(alpha[..., None] * torch.sigmoid(raw[..., :3]), -2)
    return rgb_map + (1. - alpha.sum(-1)[..., None]) if white else rgb_map


def _scan_autograd(O, raw, z, rd, g_rgb, white, noise, dtype):
    r = raw.to(dtype).clone().requires_grad_(True)
    nz = None if noise is None else noise.to(dtype)
    if z.shape[1] == 1:
        rgb = _raw2outputs_one_sample(r, rd.to(dtype), white, nz)
    else:
        rgb = O.raw2outputs(r, z.to(dtype), rd.to(dtype), white_bkgd=white, noise=nz)[0]
    (rgb * g_rgb.to(dtype)).sum().backward()
    return r.grad.detach()


def _scan_hip(L, raw, z, rd, g_rgb, white, noise, pad=64):
    """g_raw written into the middle of a NaN-filled buffer: (g_raw, the buffer's two margins)"""
    n, S = z.shape
    buf = torch.full((pad + n * S * 4 + pad,), float('nan'), device='cuda')
    dev = [t.cuda().contiguous() for t in (raw, z, rd, g_rgb)]
    nz = None if noise is None else noise.cuda().contiguous()
    out = buf[pad:pad + n * S * 4]
    rc = L.nerf_train_raw2outputs_backward(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(nz), n, S, int(white), _p(dev[3]), _p(out), _stream())
    assert rc == 0, L.r2l_last_error().decode()
    torch.cuda.synchronize()
    return out.view(n, S, 4).cpu(), torch.cat([buf[:pad], buf[pad + n * S * 4:]]).cpu()


@pytest.mark.parametrize('S', [1, 7, 64, 192])
def test_scan_backward_against_float64(L, S):
    """white_bkgd on and off, with and without noise, densities from empty rays to sigma of several hundred, rays that saturate in
    the interior: g_raw within 4 x torch-fp32's gap from float64 autograd, finite, exactly 0 where it must be, the same bits twice,
    nothing written beside [n, S, 4]"""
    from oracle import r2l_oracle as O
    n = 203
    for kind in ('thin', 'mixed', 'saturated', 'empty'):
        for white in (False, True):
            for with_noise in (False, True):
                seed = S * 8 + 4 * white + 2 * with_noise
                raw, z, rd, g_rgb = _scan_case(n, S, kind, seed)
                noise = torch.randn(n, S, generator=torch.Generator().manual_seed(seed + 1)) if with_noise else None
                if kind == 'empty' and noise is not None:
                    noise = -noise.abs()
                got, margins = _scan_hip(L, raw, z, rd, g_rgb, white, noise)
                again, _ = _scan_hip(L, raw, z, rd, g_rgb, white, noise)
                ref = _scan_autograd(O, raw, z, rd, g_rgb, white, noise, torch.float64)
                t32 = _scan_autograd(O, raw, z, rd, g_rgb, white, noise, torch.float32)
                gap_hip, gap_t32 = _rel(got, ref), _rel(t32, ref)
                ray_hip = max(_rel(got[r], ref[r]) for r in range(n))
                ray_t32 = max(_rel(t32[r], ref[r]) for r in range(n))
                if not np.isfinite(gap_t32):
                    gap_t32 = float('inf')
                if not np.isfinite(ray_t32):
                    ray_t32 = float('inf')
                print(f'S={S} {kind} white={white} noise={with_noise}: relative L2 gap from float64: HIP {gap_hip:.2e}, torch fp32 {gap_t32:.2e}; '
                      f'worst ray: HIP {ray_hip:.2e}, torch fp32 {ray_t32:.2e}')
                assert torch.isfinite(got).all()
                assert torch.isnan(margins).all()                                   # nothing written outside [n, S, 4]
                assert torch.equal(got, again)                                      # the same bits from run to run
                pre = raw[..., 3] + (noise if noise is not None else 0.)
                assert not got[..., 3][pre <= 0].any()                              # relu'(0) = 0: exactly zero
                assert not got[:, -1, 3].any()                                      # the last sample: exp(-sigma 1e10) = 0 or sigma = 0
                if kind == 'empty':
                    assert not got.any() and not ref.any()
                assert gap_hip <= 4 * gap_t32


@pytest.mark.parametrize('S', [64, 65])
def test_scan_backward_chunk_carry_against_float64(L, S):
    """One full chunk, and one sample into the second: T of sample 64 is pass 1's carry (the product scan the forward kernels
    share) and B of sample 63 is pass 2's.  Five rays (a second block with one live wave), with noise: g_raw within 4 x
    torch-fp32's gap from float64 autograd, as test_scan_backward_against_float64 holds it."""
    from oracle import r2l_oracle as O
    n = 5
    for kind in ('thin', 'mixed'):
        for white in (False, True):
            seed = 900 + S * 4 + 2 * white + (kind == 'mixed')
            raw, z, rd, g_rgb = _scan_case(n, S, kind, seed)
            noise = torch.randn(n, S, generator=torch.Generator().manual_seed(seed + 1))
            got, margins = _scan_hip(L, raw, z, rd, g_rgb, white, noise)
            ref = _scan_autograd(O, raw, z, rd, g_rgb, white, noise, torch.float64)
            t32 = _scan_autograd(O, raw, z, rd, g_rgb, white, noise, torch.float32)
            gap_hip, gap_t32 = _rel(got, ref), _rel(t32, ref)
            if not np.isfinite(gap_t32):
                gap_t32 = float('inf')
            print(f'S={S} {kind} white={white}: relative L2 gap from float64: HIP {gap_hip:.2e}, torch fp32 {gap_t32:.2e}')
            assert torch.isfinite(got).all() and torch.isnan(margins).all()
            assert gap_hip <= 4 * gap_t32


def test_scan_backward_one_sample_matches_the_forward_kernel(L, pkg):
    """S = 1: the yardstick's forward (the oracle's expressions with the 1e10 column written out) is what nerf_raw2outputs computes"""
    from efficient_nerf_amd.teacher import raw2outputs
    for white in (False, True):
        raw, z, rd, _ = _scan_case(203, 1, 'thin', 3)
        got = raw2outputs(raw.cuda(), z.cuda(), rd.cuda(), white_bkgd=white)[0].cpu()
        want = _raw2outputs_one_sample(raw.double(), rd.double(), white, None)
        assert float((got.double() - want).abs().max()) < 1e-6


def test_scan_backward_empty_batch_and_bad_arguments(L):
    assert L.nerf_train_raw2outputs_backward(None, None, None, None, 0, 64, 1, None, None, _stream()) == 0
    p = C.c_void_p(0x1000)
    assert L.nerf_train_raw2outputs_backward(p, p, p, None, 4, 0, 1, p, C.c_void_p(0x100000), None) == -1
    assert 'nerf_train_raw2outputs_backward' in L.r2l_last_error().decode()


# ---- 2. the gradients of a whole step ----------------------------------------------------------------------------------------
def _rays(n, seed, device='cpu'):
    """origins on the sphere of radius 4 (+ noise), directions towards the scene (+ noise, not normalised, as get_rays leaves them),
    target a smooth function of the ray"""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g)
    o = 4. * o / o.norm(dim=-1, keepdim=True)
    d = -o / 4. + 0.15 * torch.randn(n, 3, generator=g)
    tgt = 0.2 + 0.1 * torch.sin(2 * d + o + torch.tensor([0., 1., 2.]))
    return o.to(device), d.to(device), tgt.to(device)


def _cfg(**kw):
    c = dict(N_samples=12, N_importance=10, multires=4, multires_views=2, i_embed=0, netdepth=4, netwidth=64, netdepth_fine=4,
             netwidth_fine=64, use_viewdirs=True, white_bkgd=True, lindisp=False)
    c.update(kw)
    return c


def _states(O, tr, seed):
    """oracle.make_nerf_state for both networks of a trainer"""
    out = []
    for k, net in enumerate(tr.nets):
        out.append(O.make_nerf_state(seed * 2 + k, net.D, net.W, tr.input_ch, tr.input_ch_views, tr.output_ch, (4,), tr.use_viewdirs))
    return out[0], (out[1] if len(out) > 1 else None)


def _yardstick(O, tr, sds, rd, target, dtype):
    """loss and gradients of img2mse(rgb) + img2mse(rgb0) under torch autograd in `dtype`, from the trainer's own embedded inputs,
    depths and noise of its last step (all detached in the reference: main.py:728)"""
    last = tr.last
    n = rd.shape[0]
    prms, loss = [], 0.
    for k, sd in enumerate(sds):
        if sd is None:
            continue
        sfx = '0' if k == 0 else '1'
        prm = {key: v.detach().to('cuda', dtype).clone().requires_grad_(True) for key, v in sd.items()}
        x = last['emb' + sfx] if not tr.use_viewdirs else torch.cat([last['emb' + sfx], last['dirs' + sfx]], -1)
        raw = O.nerf_forward(prm, x.to(dtype), tr.input_ch, (4,), tr.use_viewdirs).view(n, -1, tr.raw_ch)
        nz = last['noise' + sfx]
        rgb = O.raw2outputs(raw, last['z' + sfx].to(dtype), rd.to(dtype), white_bkgd=tr.white_bkgd, noise=None if nz is None else nz.to(dtype))[0]
        loss = loss + ((rgb - target.to(dtype)) ** 2).mean()
        prms.append(prm)
    loss.backward()
    grads = [{key: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for key, v in prm.items()} for prm in prms]
    return float(loss.item()), grads


def _gaps(got, ref):
    """(global relative L2 gap over both networks' parameters, largest per-tensor gap); a tensor whose float64 gradient is zero
    must be zero"""
    num, den = {}, {}
    for k, (gn, rn) in enumerate(zip(got, ref)):
        for key in rn:
            num[k, key] = float((gn[key].double() - rn[key].double()).norm())
            den[k, key] = float(rn[key].double().norm())
            if den[k, key] == 0:
                assert num[k, key] == 0, key
    glob = np.sqrt(sum(v ** 2 for v in num.values())) / np.sqrt(sum(v ** 2 for v in den.values()))
    return glob, max(num[q] / den[q] for q in num if den[q] > 0)


def _band_check(name, hip, t32, loss_rows):
    for q, label in ((0, 'global'), (1, 'per-tensor')):
        h, t = max(r[q] for r in hip), max(r[q] for r in t32)
        print(f'{name}: {label} relative L2 gap of the gradients from float64: HIP {[f"{r[q]:.2e}" for r in hip]}, torch fp32 '
              f'{[f"{r[q]:.2e}" for r in t32]} (ratio of the maxima {h / t:.2f})')
    for lh, lt, l64 in loss_rows:
        print(f'{name}: loss f64 {l64:.9f}: |HIP - f64| / f64 = {abs(lh - l64) / l64:.2e}, torch fp32 {abs(lt - l64) / l64:.2e}')
    for q in (0, 1):
        assert max(r[q] for r in hip) <= 4 * max(r[q] for r in t32)
    for lh, lt, l64 in loss_rows:
        assert abs(lh - l64) / l64 <= max(4 * abs(lt - l64) / l64, 1e-7)


def _one_case(O, tr, seed, n, raw_noise_std=0.):
    sds = _states(O, tr, seed)
    tr.load_state_dicts(*sds)
    g = torch.Generator().manual_seed(1000 + seed)
    ro, rd, _ = _rays(n, seed, 'cuda')
    target = torch.rand(n, 3, generator=g).cuda()
    t_rand = torch.rand(n, tr.N_samples, generator=g).cuda()
    u = torch.rand(n, max(1, tr.N_importance), generator=g).cuda() if tr.N_importance > 0 else None
    noise = None
    if raw_noise_std > 0:
        noise = tuple(raw_noise_std * torch.randn(n, net.S, generator=g).cuda() for net in tr.nets)
    loss = float(tr.forward_backward(ro, rd, target, perturb=1., t_rand=t_rand, u=u, noise=noise).item())
    got = [g_ for g_ in tr.grads() if g_ is not None]
    for key in ('z0', 'z1'):                              # the depths a pass composites along are ascending (main.py:730-732 sorts)
        if key in tr.last:
            assert bool((tr.last[key][:, 1:] >= tr.last[key][:, :-1]).all()), key
    l64, g64 = _yardstick(O, tr, sds, rd, target, torch.float64)
    l32, g32 = _yardstick(O, tr, sds, rd, target, torch.float32)
    for gn, sd in zip(got, sds):
        assert list(gn) == list(sd)                       # the gradient names are the state dict's, in its order
        assert all(torch.isfinite(v).all() for v in gn.values())
    return (loss, l32, l64), _gaps(got, g64), _gaps(g32, g64), got


def test_whole_step_gradients_readme_pair(pkg):
    """8 x 256 twice, 64 + 128 samples, view directions, white background, 512 rays, seeds 0-2, jittered depths and drawn u"""
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    n = 512
    tr = NeRFTrainer(N_samples=64, N_importance=128, white_bkgd=True, max_rays=n)
    hip, t32, losses = [], [], []
    for seed in range(3):
        row, gh, gt, _ = _one_case(O, tr, seed, n)
        losses.append(row), hip.append(gh), t32.append(gt)
    _band_check('8x256 pair', hip, t32, losses)


SMALL = [
    ('D4 W128 coarse, D6 W64 fine', dict(netdepth=4, netwidth=128, netdepth_fine=6, netwidth_fine=64), 0.),
    ('no view directions (output_ch 5)', dict(use_viewdirs=False, netdepth=6, netdepth_fine=6), 0.),
    ('N_importance 0', dict(N_importance=0, netdepth=6), 0.),
    ('N_importance 0, no view directions (output_ch 4)', dict(N_importance=0, use_viewdirs=False), 0.),
    ('black background', dict(white_bkgd=False), 0.),
    ('raw_noise_std 1', dict(), 1.),
    ('i_embed -1', dict(i_embed=-1), 0.),
    ('lindisp', dict(lindisp=True, netdepth=8, netdepth_fine=7), 0.),
]


def test_whole_step_gradients_small_variants(pkg):
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    n = 300
    hip, t32, losses = [], [], []
    for case, (label, kw, std) in enumerate(SMALL):
        tr = NeRFTrainer(max_rays=n, **_cfg(**kw))
        row, gh, gt, got = _one_case(O, tr, 10 + case, n, std)
        print(f'{label}: HIP {gh[0]:.2e} / {gh[1]:.2e}, torch fp32 {gt[0]:.2e} / {gt[1]:.2e}')
        losses.append(row), hip.append(gh), t32.append(gt)
        if not tr.use_viewdirs:
            for gn in got:
                assert not gn['views_linears.0.weight'].any() and not gn['views_linears.0.bias'].any()
                if tr.output_ch == 5:
                    assert not gn['output_linear.weight'][4].any() and not gn['output_linear.bias'][4].any()
                assert gn['output_linear.weight'][:4].any()
    _band_check('small variants', hip, t32, losses)


def test_one_step_with_a_nan_in_the_coarse_noise(pkg):
    """300 rays through the smallest trainer above (4 x 64 twice, 12 + 10 samples), one NaN in the coarse pass's density noise
    (ray 100, sample 5) and nothing else poisoned.  F.relu passes the NaN on: the coarse colour of that ray, the loss and -- through
    sample_pdf on its weights -- the ray's fine depths are NaN.  The loss is NaN as float32 autograd's, and every gradient tensor of
    both networks has float32 autograd's NaN and infinity masks (float64's are the same).  A scan that renders the sample as empty
    space reports a finite loss here."""
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    n, bad = 300, 100
    tr = NeRFTrainer(max_rays=n, **_cfg())
    sds = _states(O, tr, 15)
    tr.load_state_dicts(*sds)
    g = torch.Generator().manual_seed(1015)
    ro, rd, _ = _rays(n, 15, 'cuda')
    target = torch.rand(n, 3, generator=g).cuda()
    t_rand = torch.rand(n, tr.N_samples, generator=g).cuda()
    u = torch.rand(n, tr.N_importance, generator=g).cuda()
    noise = [0.5 * torch.randn(n, net.S, generator=g) for net in tr.nets]
    noise[0][bad, 5] = float('nan')
    loss = float(tr.forward_backward(ro, rd, target, perturb=1., t_rand=t_rand, u=u, noise=tuple(t.cuda() for t in noise)).item())
    got = [g_ for g_ in tr.grads() if g_ is not None]
    others = [r for r in range(n) if r != bad]
    assert torch.isnan(tr.last['rgb0'][bad]).all() and torch.isfinite(tr.last['rgb0'][others]).all()
    assert torch.isnan(tr.last['z_samples'][bad]).all() and torch.isfinite(tr.last['z1'][others]).all()
    l32, g32 = _yardstick(O, tr, sds, rd, target, torch.float32)
    l64, g64 = _yardstick(O, tr, sds, rd, target, torch.float64)
    masks = lambda t: (torch.isnan(t), t == float('inf'), t == -float('inf'))
    assert np.isnan(l32) and np.isnan(l64) and np.isnan(loss)
    for gn, r32, r64 in zip(got, g32, g64):
        assert list(gn) == list(r32)
        for k in r32:
            assert all(torch.equal(a, b) for a, b in zip(masks(r32[k]), masks(r64[k].float()))), k      # the precondition
            assert all(torch.equal(a, b) for a, b in zip(masks(gn[k]), masks(r32[k]))), k
    assert any(torch.isnan(v).any() for v in g32[0].values())


def test_buffers_that_do_not_fit_name_their_sizes(pkg):
    from efficient_nerf_amd import R2LError
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    tr = NeRFTrainer(max_rays=1 << 22)
    with pytest.raises(R2LError) as e:
        tr.load_state_dicts(*tr.init_state_dicts(0))
    assert 'GiB' in str(e.value) and 'points x' in str(e.value) and 'N_rand' in str(e.value)


# ---- 3. a short run ----------------------------------------------------------------------------------------------------------
RUN = dict(N_samples=16, N_importance=16, multires=4, multires_views=2, netdepth=4, netwidth=64, netdepth_fine=4, netwidth_fine=64,
           use_viewdirs=True, white_bkgd=True)
N_STEP = 60
WINDOWS = [(0, 5), (5, 15), (15, 30), (30, 60)]
LR = 1e-3


def _torch_step(O, prm_c, prm_f, cfg, z_coarse, ro, rd, tgt, t_rand, u):
    """render_rays (main.py:624-756) with perturb = 1 and given draws + the two losses, under autograd"""
    n = ro.shape[0]
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    net = dict(multires=cfg['multires'], multires_views=cfg['multires_views'], i_embed=0, use_viewdirs=True)
    z0 = O.perturb_z_vals(z_coarse.expand(n, -1), t_rand=t_rand)
    raw0 = O.run_network_generic(prm_c, ro[:, None, :] + rd[:, None, :] * z0[:, :, None], vd, **net)
    rgb0, _, _, w0, _ = O.raw2outputs(raw0, z0, rd, white_bkgd=cfg['white_bkgd'])
    z_mid = .5 * (z0[:, 1:] + z0[:, :-1])
    z_s = O.sample_pdf(z_mid, w0[:, 1:-1], cfg['N_importance'], det=False, u=u).detach()
    z1 = O.merge_z(z0, z_s)
    raw1 = O.run_network_generic(prm_f, ro[:, None, :] + rd[:, None, :] * z1[:, :, None], vd, **net)
    rgb = O.raw2outputs(raw1, z1, rd, white_bkgd=cfg['white_bkgd'])[0]
    return ((rgb0 - tgt) ** 2).mean() + ((rgb - tgt) ** 2).mean()


def _permute_hidden(sd, seed):
    """the same network with the hidden units behind pts_linears.0 permuted: another fp32 summation order"""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    perm = torch.randperm(sd['pts_linears.0.weight'].shape[0], generator=g)
    out['pts_linears.0.weight'], out['pts_linears.0.bias'] = sd['pts_linears.0.weight'][perm], sd['pts_linears.0.bias'][perm]
    out['pts_linears.1.weight'] = sd['pts_linears.1.weight'][:, perm]
    return out


def test_short_training_run(pkg):
    """60 Adam steps at 256 rays per step on an analytic scene (6 batches of rays around a sphere, colours a smooth function of the
    ray): the HIP loss curve stays as close to torch autograd's on the GPU (A, same draws) as the same networks in another fp32
    summation order do (B), window by window, factor 4; A falls by >= 4 x (else the set-up does not train), HIP by >= 2 x; a
    second HIP run gives the same bits."""
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    n, n_batch = 256, 6
    pool = [_rays(n, 300 + b, 'cuda') for b in range(n_batch)]
    g = torch.Generator().manual_seed(9)
    order = torch.randint(0, n_batch, (N_STEP,), generator=g).tolist()
    t_rands = [torch.rand(n, RUN['N_samples'], generator=g).cuda() for _ in range(N_STEP)]
    us = [torch.rand(n, RUN['N_importance'], generator=g).cuda() for _ in range(N_STEP)]
    tr = NeRFTrainer(max_rays=n, **RUN)
    sd_c, sd_f = _states(O, tr, 21)

    def run_hip():
        tr.load_state_dicts(sd_c, sd_f)
        tr.load_optimizer_state_dict({'state': {}, 'param_groups': tr.optimizer_state_dict()['param_groups']})
        losses = []
        for t in range(N_STEP):
            ro, rd, tgt = pool[order[t]]
            loss, _ = tr.step(ro, rd, tgt, LR, perturb=1., t_rand=t_rands[t], u=us[t])
            losses.append(loss.clone())
        return torch.cat(losses).cpu(), tr.state_dicts()

    H1, sds1 = run_hip()
    H2, sds2 = run_hip()
    assert torch.equal(H1, H2)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(sds1, sds2) for k in a)            # bit-identical from run to run

    def run_torch(sd_c, sd_f):
        prm_c = {k: v.detach().cuda().clone().requires_grad_(True) for k, v in sd_c.items()}
        prm_f = {k: v.detach().cuda().clone().requires_grad_(True) for k, v in sd_f.items()}
        opt = torch.optim.Adam(list(prm_c.values()) + list(prm_f.values()), lr=LR, betas=(0.9, 0.999))
        z_coarse = tr.z_coarse.cuda()
        losses = []
        for t in range(N_STEP):
            ro, rd, tgt = pool[order[t]]
            loss = _torch_step(O, prm_c, prm_f, RUN, z_coarse, ro, rd, tgt, t_rands[t], us[t])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach().reshape(1))
        return torch.cat(losses).cpu()

    A = run_torch(sd_c, sd_f).double()
    B = run_torch(_permute_hidden(sd_c, 77), _permute_hidden(sd_f, 78)).double()
    H = H1.double()
    first, last = WINDOWS[0], WINDOWS[-1]
    fall = lambda X: float(X[first[0]:first[1]].mean() / X[last[0]:last[1]].mean())
    print(f'mean loss of steps {first} -> {last}: A {A[first[0]:first[1]].mean():.5f} -> {A[last[0]:last[1]].mean():.5f} (1/{fall(A):.1f}), '
          f'HIP 1/{fall(H):.1f}')
    # the running band starts at one fp32 spacing (2^-23 relative): the losses are fp32 numbers, and two correct runs whose losses
    # differ in the last bit must not fail where A and B happen to agree bit for bit (a zero band)
    band, rows = 2.0 ** -23, []
    for a, b in WINDOWS:
        d_h = float(((H[a:b] - A[a:b]).abs() / A[a:b]).max())
        d_b = float(((B[a:b] - A[a:b]).abs() / A[a:b]).max())
        band = max(band, d_b)
        rows.append((a, b, d_h, band))
        print(f'steps [{a}, {b}): d(HIP) = {d_h:.2e}, d(B) = {d_b:.2e}, band so far {band:.2e}')
    assert fall(A) >= 4, 'the set-up does not train'
    for a, b, d_h, bnd in rows:
        assert d_h <= 4 * bnd, (a, b, d_h, bnd)
    assert fall(H) >= 2


# ---- 4. optimizer state interchange ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_viewdirs', [True, False])
def test_optimizer_state_interchange_with_torch_adam(pkg, use_viewdirs):
    """three HIP steps, the state into a torch.optim.Adam over the parameters in the reference's order (coarse, then fine), one
    given gradient applied on both sides: as close as Adam alone (tests/test_train_gpu.py::test_adam_against_float64); torch's
    state loads back.  Without view directions views_linears.0 has no state and does not move."""
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    n = 200
    cfg = _cfg(use_viewdirs=use_viewdirs)
    tr = NeRFTrainer(max_rays=n, **cfg)
    tr.load_state_dicts(*_states(O, tr, 5))
    before = tr.state_dicts()
    ro, rd, tgt = _rays(n, 8, 'cuda')
    for k in range(3):
        tr.step(ro, rd, tgt, 1e-3 * (k + 1))
    osd = tr.optimizer_state_dict()
    names = tr.state_names()
    live = [i for i, k in enumerate(names) if k not in tr._frozen]
    assert sorted(osd['state']) == live and all(float(s['step']) == 3 for s in osd['state'].values())
    assert len(live) == len(names) - (0 if use_viewdirs else 4)
    sd = dict(zip(names, [v for part in tr.state_dicts() for v in part.values()]))
    assert list(sd) == [f'{p}.{k}' for p, part in zip(('network_fn', 'network_fine'), tr.state_dicts()) for k in part]
    if not use_viewdirs:
        for part, part0 in zip(tr.state_dicts(), before):
            assert torch.equal(part['views_linears.0.weight'], part0['views_linears.0.weight'])
            assert not torch.equal(part['pts_linears.0.weight'], part0['pts_linears.0.weight'])
    g = torch.Generator().manual_seed(3)
    given = {k: torch.randn(v.shape, generator=g) * 10 ** (-6 * torch.rand(v.shape, generator=g)) for k, v in sd.items()}
    lr = 7e-4
    outs = {}
    for dtype in (torch.float64, torch.float32):
        prm = [torch.nn.Parameter(v.to(dtype).clone()) for v in sd.values()]
        opt = torch.optim.Adam(prm, lr=1.0, betas=(0.9, 0.999))
        opt.load_state_dict(tr.optimizer_state_dict())
        assert opt.param_groups[0]['lr'] == 3e-3
        opt.param_groups[0]['lr'] = lr
        for p_, k in zip(prm, sd):
            if k not in tr._frozen:
                p_.grad = given[k].to(dtype)
        opt.step()
        outs[dtype] = {k: p_.detach() for p_, k in zip(prm, sd)}
        if dtype == torch.float32:
            tr2 = NeRFTrainer(max_rays=n, **cfg)
            cut = lambda pre: {k[len(pre) + 1:]: v for k, v in outs[dtype].items() if k.startswith(pre + '.')}
            tr2.load_state_dicts(cut('network_fn'), cut('network_fine')).load_optimizer_state_dict(opt.state_dict())
            assert tr2.t == 4
            assert all(torch.equal(tr2.exp_avg[k].cpu(), opt.state[p_]['exp_avg']) for p_, k in zip(prm, sd) if k not in tr._frozen)
    for k, v in given.items():
        tr.g[k].copy_(torch.zeros_like(v) if k in tr._frozen else v)
    tr.adam(lr)
    hip = dict(zip(names, [v for part in tr.state_dicts() for v in part.values()]))
    gap_hip = max(float((hip[k].double() - outs[torch.float64][k]).abs().max()) for k in sd)
    gap_t32 = max(float((outs[torch.float32][k].double() - outs[torch.float64][k]).abs().max()) for k in sd)
    print(f'state interchange: max|p_hip - p_f64| = {gap_hip:.3e}, max|p_torch_fp32 - p_f64| = {gap_t32:.3e}')
    assert gap_hip <= 4 * gap_t32


# ---- 5. command line ---------------------------------------------------------------------------------------------------------
def write_scene(root, n_train=6, n_test=2, side=64):
    """a Blender-layout scene: RGBA PNGs whose colours are a smooth function of the ray (opaque everywhere), transforms_*.json"""
    from efficient_nerf_amd import frontend as fe
    from oracle import r2l_oracle as O
    angle = O.LEGO_CAMERA_ANGLE_X
    focal = O.focal_from_angle(side, angle)
    k = 0
    for split, count in (('train', n_train), ('val', 1), ('test', n_test)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i in range(count):
            c2w = O.pose_spherical(-180. + 47. * k, -30. + 5. * (k % 3), 4.)
            k += 1
            ro, rd = O.get_rays(side, side, focal, c2w[:3, :4])
            rgb = 0.2 + 0.1 * torch.sin(2 * rd + ro + torch.tensor([0., 1., 2.]))
            img = torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1).reshape(side, side, 4)
            fe.write_png(os.path.join(root, split, f'r_{i}.png'), fe.to8b(img.numpy()))
            frames.append(dict(file_path=f'./{split}/r_{i}', transform_matrix=c2w.tolist()))
        with open(os.path.join(root, f'transforms_{split}.json'), 'w') as fp:
            json.dump(dict(camera_angle_x=angle, frames=frames), fp)


def _run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_trains_tests_saves_renders_and_resumes(pkg, tmp_path):
    """train_teacher.py with configs/lego.txt as a child process on a small scene written here; main.py --render_only on its
    checkpoint; --resume from it.  Each child under its own timeout; a failure starts nothing further.
    The children train under --dist_seed 0: unseeded, about one start in eight (of seeds 0 .. 5: seed 4) draws weights whose density is zero
    on every sample, renders white at 2 dB and does not move in 30 iterations, as the reference's own initialisation can; `hist_psnr` then
    wanders instead of rising (2.18 -> 2.12 in the run that showed it).  With the seed the run is the same every time: 11.9 -> 20.7 dB."""
    scene = str(tmp_path / 'scene')
    write_scene(scene)
    base = ['--config', os.path.join(ROOT, 'configs', 'lego.txt'), '--datadir', scene, '--basedir', str(tmp_path), '--expname', 'cli',
            '--N_rand', '128', '--testskip', '1']
    train = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'train_teacher.py')] + base + [
        '--lrate', '0.002', '--precrop_iters', '10', '--i_print', '5', '--i_weights', '15', '--i_video', '100000', '--dist_seed', '0']
    out = _run(train + ['--N_iters', '30', '--i_testset', '30'], str(tmp_path))
    lines = [ln for ln in out.splitlines() if ln.startswith('[TRAIN] Iter')]
    assert len(lines) == 6, out[-3000:]
    assert all(re.fullmatch(r'\[TRAIN\] Iter \d+ data_time \d+\.\d{4} batch_time \d+\.\d{4} loss \d+\.\d{6} psnr \S+ hist_psnr \S+ LR \d\.\d{10}', ln)
               for ln in lines), lines
    hist = [float(re.search(r'hist_psnr (\S+)', ln).group(1)) for ln in lines]
    assert hist[-1] > hist[0], hist
    assert 'Center cropping of size 16 x 16 is enabled until iter 10' in out
    tests = [ln for ln in out.splitlines() if ln.startswith('[TEST] Iter')]
    assert len(tests) == 1 and re.match(r'\[TEST\] Iter 30 TestPSNR \S+ TestPSNRv2 \S+ BestPSNRv2 \S+ \(Iter 30\)', tests[0]), tests
    wdir = tmp_path / 'cli' / 'weights'
    for name in ('ckpt.tar', 'ckpt_best.tar'):
        saved = torch.load(str(wdir / name), map_location='cpu', weights_only=False)
        assert {'network_fn_state_dict', 'network_fine_state_dict', 'optimizer_state_dict', 'global_step', 'best_psnr', 'best_psnr_step'} <= set(saved)
        assert saved['global_step'] == 30 and len(saved['optimizer_state_dict']['state']) == 2 * 24
        assert list(saved['network_fn_state_dict'])[16:18] == ['views_linears.0.weight', 'views_linears.0.bias']
    ck = str(wdir / 'ckpt.tar')
    outdir = str(tmp_path / 'render')
    _run(['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'main.py'), '--model_name', 'nerf'] + base + [
        '--pretrained_ckpt', ck, '--render_only', '--synthetic_poses', '1', '--H', '32', '--outdir', outdir], str(tmp_path))
    rgbs = np.load(os.path.join(outdir, 'rgbs.npy'))
    assert rgbs.shape[-1] == 3 and np.isfinite(rgbs).all()
    out = _run(train + ['--N_iters', '40', '--i_testset', '1000', '--pretrained_ckpt', ck, '--resume'], str(tmp_path))
    assert 'Resume optimizer successfully.' in out
    its = [int(re.search(r'Iter (\d+)', ln).group(1)) for ln in out.splitlines() if ln.startswith('[TRAIN] Iter')]
    assert its == [35, 40], out[-2000:]
    assert torch.load(ck, map_location='cpu', weights_only=False)['global_step'] == 40

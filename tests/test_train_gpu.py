"""GPU: training of the R2L student in the library's fp32 kernels (csrc/r2l_train.hip, efficient-nerf_amd/train.py).

Yardsticks: float64 matmul with a derived rounding bound for the two backward GEMMs and the element-wise pass; for everything
that crosses ReLUs (whole-network gradients, training runs) float64 autograd of oracle/r2l_oracle.py's forward functions, with the
band torch's own fp32 keeps from it, measured in the same test, as the scale (factor 4: another fp32 summation order, nothing
more)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24          # fp32 unit roundoff


def gamma(m):
    return m * U / (1 - m * U)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope='module')
def L(pkg, built_lib):
    from efficient_nerf_amd import _lib
    return _lib.lib()


def _check(L, rc):
    assert rc == 0, L.r2l_last_error().decode()


def _grad_weight(L, gz, x, out_dim, in_dim):
    n = x.shape[0]
    slabs = L.r2l_train_grad_weight_slabs(n)
    ws = torch.full((max(1, slabs * (out_dim * in_dim + out_dim)),), float('nan'), device='cuda')
    gw = torch.full((out_dim, in_dim), float('nan'), device='cuda')
    gb = torch.full((out_dim,), float('nan'), device='cuda')
    _check(L, L.r2l_train_grad_weight(_p(gz), out_dim, _p(x), in_dim, n, out_dim, in_dim, _p(gw), _p(gb), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    return gw, gb, slabs


# ---- 1. the two backward GEMMs and the element-wise pass, against float64 ----------------------------------------------------
@pytest.mark.parametrize('n,in_dim,out_dim', [(1, 256, 256), (300, 1008, 256), (4133, 256, 3), (8192, 256, 256), (0, 256, 256)])
def test_backward_gemms_against_float64(L, n, in_dim, out_dim):
    """|hip - f64| <= gamma_m (|A| |B|) elementwise, m = reduction length + slabs + 2: the MFMA is a k-ordered fp32 fmaf chain
    and the slab pass adds one addition per slab."""
    g = torch.Generator().manual_seed(n + in_dim)
    gz, x, w = torch.randn(n, out_dim, generator=g), torch.randn(n, in_dim, generator=g), torch.randn(out_dim, in_dim, generator=g) / 16
    gzd, xd, wd = gz.cuda(), x.cuda(), w.cuda()
    # g_x = g_z W
    gx = torch.full((n, in_dim), float('nan'), device='cuda')
    _check(L, L.r2l_train_grad_input(_p(gzd), out_dim, n, _p(wd), out_dim, in_dim, _p(gx), in_dim, 0, _stream()))
    ref, mag = gz.double() @ w.double(), gz.double().abs() @ w.double().abs()
    dx = (gx.cpu().double() - ref).abs()
    print(f'g_x n={n} {in_dim}->{out_dim}: max err / bound = {float((dx / (gamma(out_dim + 2) * mag + 1e-300)).max()) if n else 0:.3f}')
    assert torch.isfinite(gx).all() and bool((dx <= gamma(out_dim + 2) * mag).all())
    # ... on top of what the destination holds (the accumulate flag): one more addition
    c0 = torch.randn(n, in_dim, generator=g)
    gx2 = c0.cuda()
    _check(L, L.r2l_train_grad_input(_p(gzd), out_dim, n, _p(wd), out_dim, in_dim, _p(gx2), in_dim, 1, _stream()))
    d2 = (gx2.cpu().double() - (ref + c0.double())).abs()
    assert bool((d2 <= gamma(out_dim + 3) * (mag + c0.double().abs())).all())
    # g_W = g_z^T x, g_b = column sums of g_z
    gw, gb, slabs = _grad_weight(L, gzd, xd, out_dim, in_dim)
    m = n + slabs + 2
    refw, magw = gz.double().t() @ x.double(), gz.double().abs().t() @ x.double().abs()
    dw = (gw.cpu().double() - refw).abs()
    db = (gb.cpu().double() - gz.double().sum(0)).abs()
    print(f'g_W n={n} {in_dim}->{out_dim}: {slabs} slabs, max err / bound = {float((dw / (gamma(m) * magw + 1e-300)).max()) if n else 0:.3f}')
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
    assert bool((dw <= gamma(m) * magw).all()) and bool((db <= gamma(m) * gz.double().abs().sum(0)).all())
    if n == 0:
        assert not gw.any() and not gb.any()
    # two runs: the same bits
    gw_b, gb_b, _ = _grad_weight(L, gzd, xd, out_dim, in_dim)
    assert torch.equal(gw, gw_b) and torch.equal(gb, gb_b)


def test_grad_input_and_weight_on_strided_views(L):
    """column slices of wider buffers (row strides larger than the widths), as the layer-wise widths use them"""
    g = torch.Generator().manual_seed(5)
    n, in_dim, out_dim, ld = 77, 40, 24, 64
    gzb, xb, gxb = (torch.randn(n, ld, generator=g).cuda() for _ in range(3))
    w = (torch.randn(out_dim, in_dim, generator=g) / 8).cuda()
    keep = gxb.clone()
    _check(L, L.r2l_train_grad_input(_p(gzb), ld, n, _p(w), out_dim, in_dim, _p(gxb), ld, 0, _stream()))
    ref = gzb[:, :out_dim].cpu().double() @ w.cpu().double()
    mag = gzb[:, :out_dim].cpu().double().abs() @ w.cpu().double().abs()
    assert bool(((gxb[:, :in_dim].cpu().double() - ref).abs() <= gamma(out_dim + 2) * mag).all())
    assert torch.equal(gxb[:, in_dim:], keep[:, in_dim:])             # nothing written beside the view
    slabs = L.r2l_train_grad_weight_slabs(n)
    ws = torch.empty(slabs * (out_dim * in_dim + out_dim), device='cuda')
    gw, gb = torch.empty(out_dim, in_dim, device='cuda'), torch.empty(out_dim, device='cuda')
    _check(L, L.r2l_train_grad_weight(_p(gzb), ld, _p(xb), ld, n, out_dim, in_dim, _p(gw), _p(gb), _p(ws), ws.numel(), _stream()))
    refw = gzb[:, :out_dim].cpu().double().t() @ xb[:, :in_dim].cpu().double()
    magw = gzb[:, :out_dim].cpu().double().abs().t() @ xb[:, :in_dim].cpu().double().abs()
    assert bool(((gw.cpu().double() - refw).abs() <= gamma(n + slabs + 2) * magw).all())


@pytest.mark.parametrize('act', ['none', 'relu', 'lrelu', 'sigmoid'])
@pytest.mark.parametrize('scale', [1.0, 0.5])
def test_act_backward_against_float64(L, act, scale):
    """g_post (+)= g_y; g_u = g_y act'(y - post); g_res (+)= g_u; g_z = scale g_u -- three roundings at most per output"""
    code = {'none': 0, 'relu': 1, 'lrelu': 2, 'sigmoid': 3}[act]
    g = torch.Generator().manual_seed(code)
    n, w = 301, 50
    u = torch.randn(n, w, generator=g)
    a = {'none': u, 'relu': torch.relu(u), 'lrelu': torch.nn.functional.leaky_relu(u), 'sigmoid': torch.sigmoid(u)}[act]
    gy = torch.randn(n, w, generator=g)
    for with_post in ((False, True) if act != 'sigmoid' else (False,)):
        post = torch.randn(n, w, generator=g) if with_post else None
        y = a + post if with_post else a
        a64 = y.double() - post.double() if with_post else y.double()
        d64 = {'none': torch.ones_like(a64), 'relu': (a64 > 0).double(), 'lrelu': torch.where(a64 > 0, 1.0, 0.01).double(), 'sigmoid': a64 * (1 - a64)}[act]
        gu64 = gy.double() * d64
        gy_d, y_d, post_d = gy.cuda(), y.cuda(), post.cuda() if with_post else None
        res0, post0 = torch.randn(n, w, generator=g), torch.randn(n, w, generator=g)
        for res_acc in (0, 1):
            gz = torch.full((n, w), float('nan'), device='cuda')
            gres, gpost = res0.cuda(), post0.cuda()
            _check(L, L.r2l_train_act_backward(_p(gy_d), w, _p(y_d), w, _p(post_d), w, n, w, code,
                                               scale, _p(gz), w, _p(gres), w, res_acc, _p(gpost), w, 0, _stream()))
            assert torch.equal(gpost.cpu(), gy)
            assert bool(((gz.cpu().double() - scale * gu64).abs() <= gamma(4) * (scale * gu64).abs()).all())
            want = gu64 + (res0.double() if res_acc else 0)
            assert bool(((gres.cpu().double() - want).abs() <= gamma(4) * (gu64.abs() + (res0.double().abs() if res_acc else 0))).all())
        # in place (g_res over g_y) and g_post = g_res (a one-block body): g_y + g_u
        gyd = gy.cuda()
        gz = torch.empty((n, w), device='cuda')
        _check(L, L.r2l_train_act_backward(_p(gyd), w, _p(y_d), w, _p(post_d), w, n, w, code, scale,
                                           _p(gz), w, _p(gyd), w, 0, None, 0, 0, _stream()))
        assert bool(((gyd.cpu().double() - gu64).abs() <= gamma(4) * gu64.abs()).all())
        both = torch.zeros((n, w), device='cuda')
        _check(L, L.r2l_train_act_backward(_p(gy_d), w, _p(y_d), w, _p(post_d), w, n, w, code, scale,
                                           _p(gz), w, _p(both), w, 1, _p(both), w, 0, _stream()))
        assert bool(((both.cpu().double() - (gy.double() + gu64)).abs() <= gamma(4) * (gy.double().abs() + gu64.abs())).all())


def test_mse_loss_against_float64(L):
    g = torch.Generator().manual_seed(2)
    for n in (1, 255, 4133):
        rgb, tgt = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
        for through in (0, 1):
            gout, err, loss = torch.empty(n, 3, device='cuda'), torch.empty(n, device='cuda'), torch.empty(1, device='cuda')
            ws = torch.empty((n + 255) // 256, device='cuda')
            rgb_d, tgt_d = rgb.cuda(), tgt.cuda()
            _check(L, L.r2l_train_mse_loss(_p(rgb_d), _p(tgt_d), n, through, _p(gout), _p(err), _p(loss), _p(ws), ws.numel(), _stream()))
            d = rgb.double() - tgt.double()
            want_g = 2 * d / (3 * n) * (rgb.double() * (1 - rgb.double()) if through else 1)
            assert abs(loss.item() - float((d ** 2).mean())) <= gamma(n + 600) * float((d ** 2).mean())
            assert bool(((gout.cpu().double() - want_g).abs() <= gamma(8) * want_g.abs() + 1e-45).all())
            assert bool(((err.cpu().double() - (d ** 2).mean(1)).abs() <= gamma(8) * (d ** 2).mean(1) + 1e-45).all())


# ---- 2. Adam alone -----------------------------------------------------------------------------------------------------------
def _torch_adam_run(p0, grads, lrs, dtype, state=None):
    prm = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adam([prm], lr=1.0, betas=(0.9, 0.999))
    if state is not None:
        opt.load_state_dict(state)
    for gr, lr in zip(grads, lrs):
        opt.param_groups[0]['lr'] = lr
        prm.grad = gr.to(dtype).clone()
        opt.step()
    return prm.detach()


def test_adam_against_float64(L):
    """10 steps on 4,096 parameters, gradient magnitudes over 1e-9 ... 1, another lr every step: no further from torch's float64
    Adam than 4 x torch's own fp32 Adam is"""
    g = torch.Generator().manual_seed(11)
    n = 4096
    p0 = torch.randn(n, generator=g)
    mags = 10 ** (-9 * torch.rand(n, generator=g))
    grads = [torch.randn(n, generator=g) * mags for _ in range(10)]
    lrs = [1e-4 + 4e-5 * k for k in range(10)]
    p64 = _torch_adam_run(p0, grads, lrs, torch.float64)
    p32 = _torch_adam_run(p0, grads, lrs, torch.float32)
    p, m, v = p0.cuda(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    for k, (gr, lr) in enumerate(zip(grads, lrs)):
        gr_d = gr.cuda()
        _check(L, L.r2l_train_adam(_p(p), _p(gr_d), _p(m), _p(v), n, lr, k + 1, _stream()))
    gap_hip = float((p.cpu().double() - p64).abs().max())
    gap_t32 = float((p32.double() - p64).abs().max())
    print(f'Adam: max|p_hip - p_f64| = {gap_hip:.3e}, max|p_torch_fp32 - p_f64| = {gap_t32:.3e} (ratio {gap_hip / gap_t32:.2f})')
    assert gap_hip <= 4 * gap_t32


# ---- 3. whole-network gradients ----------------------------------------------------------------------------------------------
def _rays(n, seed, device='cpu'):
    """origins (0, 0, 4) + 0.2 N(0, 1), directions normalize(-o + 0.8 N(0, 1)), target 0.5 + 0.5 sin(3 d + 2 o + (0, 1, 2))"""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)
    d = -o + 0.8 * torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    tgt = 0.5 + 0.5 * torch.sin(3 * d + 2 * o + torch.tensor([0., 1., 2.]))
    return o.to(device), d.to(device), tgt.to(device)


def _autograd(forward, sd, emb, target, dtype):
    """loss and gradients of mean((forward(sd, emb) - target)^2) under torch autograd in `dtype`"""
    prm = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    loss = ((forward(prm, emb.to(dtype)) - target.to(dtype)) ** 2).mean()
    loss.backward()
    return loss.item(), {k: v.grad.detach() for k, v in prm.items()}


def _gaps(got, ref):
    """(global relative L2 gap over all parameters, largest per-tensor relative L2 gap) from the float64 gradients"""
    num = {k: float((got[k].double().cpu() - ref[k]).norm()) for k in ref}
    den = {k: float(ref[k].norm()) for k in ref}
    glob = np.sqrt(sum(v ** 2 for v in num.values())) / np.sqrt(sum(v ** 2 for v in den.values()))
    return glob, max(num[k] / den[k] for k in ref)


def _band_check(name, hip, t32, loss_rows):
    """hip / t32: lists of (global gap, per-tensor gap) per case; loss_rows: (L_hip, L_t32, L_f64) per case"""
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


def test_whole_network_gradients_w256d88(pkg):
    """W256D88, seeds 0-3, 2,048 rays, jittered depths from a given t_rand, random targets: float64 autograd of the forward
    function of oracle/r2l_oracle.py as the yardstick, torch fp32 on the CPU as the band"""
    from efficient_nerf_amd.train import R2LTrainer
    from oracle import r2l_oracle as O
    n = 2048
    tr = R2LTrainer(netdepth=88, netwidth=256, use_residual=True, trial=dict(body_arch='resmlp'), max_rays=n)
    hip, t32, losses = [], [], []
    fwd = lambda prm, x: O.r2l_forward(prm, x, dtype=x.dtype)
    for seed in range(4):
        sd = O.make_r2l_state(seed)
        tr.load_state_dict(sd)
        g = torch.Generator().manual_seed(100 + seed)
        ro, rd, _ = _rays(n, seed)
        target, t_rand = torch.rand(n, 3, generator=g), torch.rand(n, 16, generator=g)
        emb = tr.embed(ro.cuda(), rd.cuda(), 1., t_rand.cuda()).cpu()
        loss = tr.forward_backward(ro.cuda(), rd.cuda(), target.cuda(), 1., t_rand.cuda()).item()
        l64, g64 = _autograd(fwd, sd, emb, target, torch.float64)
        l32, g32 = _autograd(fwd, sd, emb, target, torch.float32)
        hip.append(_gaps(tr.grads(), g64))
        t32.append(_gaps(g32, g64))
        losses.append((loss, l32, l64))
    _band_check('W256D88', hip, t32, losses)


SMALL = [
    # netdepth, netwidth, layerwise_netwidths, act, use_residual, trial
    (8, 96, '', 'relu', True, dict(body_arch='resmlp', n_block=2, n_learnable=3, res_scale=0.5, inact='lrelu', outact='none')),
    (6, 64, '', 'lrelu', False, dict(body_arch='resmlp', n_learnable=2, res_scale=1.0, inact='relu', outact='relu')),
    (6, 48, '', 'relu', True, None),
    (6, 64, '64,48,48,32,64', 'lrelu', True, None),
    (4, 32, '', 'relu', True, dict(body_arch='resmlp', n_block=1, n_learnable=2, res_scale=0.5, inact='relu', outact='lrelu')),
    (5, 40, '', 'relu', False, dict(body_arch='resmlp', n_block=2, n_learnable=1, res_scale=1.0, inact='relu', outact='none')),
]


def test_whole_network_gradients_small_variants(pkg):
    """the same band at 300 rays on small networks of v3_2_plan: lrelu, outact relu, res_scale 0.5, n_learnable 3 (and 1), a plain
    MLP body, no --use_residual, --layerwise_netwidths, a single block"""
    from efficient_nerf_amd.train import R2LTrainer
    from oracle import r2l_oracle as O
    n, n_sample, Lf = 300, 4, 3
    hip, t32, losses = [], [], []
    for case, (D, W, lw, act, use_res, trial) in enumerate(SMALL):
        tr = R2LTrainer(n_sample=n_sample, L=Lf, netdepth=D, netwidth=W, layerwise_netwidths=lw, act=act, use_residual=use_res,
                        trial=trial, max_rays=n)
        sd = O.make_v3_2_state(case, D, W, tr.input_dim, lw, act, trial)
        tr.load_state_dict(sd)
        g = torch.Generator().manual_seed(200 + case)
        ro, rd, _ = _rays(n, 50 + case)
        target, t_rand = torch.rand(n, 3, generator=g), torch.rand(n, n_sample, generator=g)
        emb = tr.embed(ro.cuda(), rd.cuda(), 1., t_rand.cuda()).cpu()
        loss = tr.forward_backward(ro.cuda(), rd.cuda(), target.cuda(), 1., t_rand.cuda()).item()
        fwd = lambda prm, x: O.v3_2_forward(prm, x, D, act, use_res, trial)
        l64, g64 = _autograd(fwd, sd, emb, target, torch.float64)
        l32, g32 = _autograd(fwd, sd, emb, target, torch.float32)
        assert set(tr.grads()) == set(g64)
        hip.append(_gaps(tr.grads(), g64))
        t32.append(_gaps(g32, g64))
        losses.append((loss, l32, l64))
    _band_check('small variants', hip, t32, losses)


def test_one_step_with_a_nan_ray(pkg):
    """257 rays through the smallest network above (4 layers of 32, one block), ray 100's origin NaN -- the row r2l_rays_from_images
    writes for an index outside the images: the loss is NaN, as float32 autograd's, and every gradient tensor has float32
    autograd's NaN and infinity masks (float64's are the same); the per-ray error is NaN on that ray alone"""
    from efficient_nerf_amd.train import R2LTrainer
    from oracle import r2l_oracle as O
    n, n_sample, Lf, bad = 257, 4, 3, 100
    D, W, lw, act, use_res, trial = SMALL[4]
    tr = R2LTrainer(n_sample=n_sample, L=Lf, netdepth=D, netwidth=W, layerwise_netwidths=lw, act=act, use_residual=use_res, trial=trial,
                    max_rays=n)
    sd = O.make_v3_2_state(4, D, W, tr.input_dim, lw, act, trial)
    tr.load_state_dict(sd)
    g = torch.Generator().manual_seed(204)
    ro, rd, _ = _rays(n, 54)
    ro[bad] = float('nan')
    target, t_rand = torch.rand(n, 3, generator=g), torch.rand(n, n_sample, generator=g)
    emb = tr.embed(ro.cuda(), rd.cuda(), 1., t_rand.cuda()).cpu()
    assert torch.isnan(emb[bad]).any() and torch.isfinite(emb[[r for r in range(n) if r != bad]]).all()
    loss = tr.forward_backward(ro.cuda(), rd.cuda(), target.cuda(), 1., t_rand.cuda()).item()
    fwd = lambda prm, x: O.v3_2_forward(prm, x, D, act, use_res, trial)
    l32, g32 = _autograd(fwd, sd, emb, target, torch.float32)
    l64, g64 = _autograd(fwd, sd, emb, target, torch.float64)
    masks = lambda t: (torch.isnan(t), t == float('inf'), t == -float('inf'))
    got = tr.grads()
    assert np.isnan(l32) and np.isnan(l64) and np.isnan(loss)
    assert set(got) == set(g32)
    for k in g32:
        assert all(torch.equal(a, b) for a, b in zip(masks(g32[k]), masks(g64[k].float()))), k      # the precondition
        assert all(torch.equal(a, b) for a, b in zip(masks(got[k].cpu()), masks(g32[k]))), k
    assert any(torch.isnan(v).any() for v in g32.values())
    err = tr._err[:n].cpu()
    assert torch.isnan(err[bad]) and torch.isfinite(err[[r for r in range(n) if r != bad]]).all()


# ---- 4. jitter ---------------------------------------------------------------------------------------------------------------
def test_sample_train_jitter_bit_equal(pkg):
    from efficient_nerf_amd import PointSampler
    from oracle import r2l_oracle as O
    for n, S in ((1, 16), (333, 16), (100, 5), (7, 1)):
        ro, rd, _ = _rays(n, n)
        t_rand = torch.rand(n, S, generator=torch.Generator().manual_seed(S))
        z_vals = O.sampler_z_vals(S, 2., 6.)
        z = O.perturb_z_vals(z_vals[None, :].expand(n, S), t_rand=t_rand)
        want = (ro[..., None, :] + rd[..., None, :] * z[..., :, None]).reshape(n, -1)      # O.sample_rays' arithmetic with per-ray depths
        got = PointSampler(8, 8, 10., S, 2., 6.).sample_train(ro.cuda(), rd.cuda(), perturb=1., t_rand=t_rand.cuda())
        assert torch.equal(got.cpu(), want)
    ro, rd, _ = _rays(64, 1)
    flat = O.sample_rays(ro, rd, O.sampler_z_vals(16, 2., 6.))
    drawn = PointSampler(8, 8, 10., 16, 2., 6.).sample_train(ro.cuda(), rd.cuda(), perturb=1.).cpu()     # the default: a torch.rand draw
    assert drawn.shape == flat.shape and torch.isfinite(drawn).all() and not torch.equal(drawn, flat)


# ---- 5. a short training run -------------------------------------------------------------------------------------------------
def _permute_blocks(sd, seed=77):
    """the same network with the hidden units of every block permuted: another fp32 summation order"""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    b = 0
    while f'body.{b}.body.0.weight' in sd:
        perm = torch.randperm(sd[f'body.{b}.body.0.weight'].shape[0], generator=g)
        out[f'body.{b}.body.0.weight'] = sd[f'body.{b}.body.0.weight'][perm]
        out[f'body.{b}.body.0.bias'] = sd[f'body.{b}.body.0.bias'][perm]
        out[f'body.{b}.body.2.weight'] = sd[f'body.{b}.body.2.weight'][:, perm]
        b += 1
    return out


N_STEP = 100
WINDOWS = [(1, 5), (5, 20), (20, 50), (50, 100)]


def test_short_training_run(pkg):
    """100 Adam steps on W256D88 (seed 21), a pool of 8 batches of 2,048 rays: the HIP loss curve stays as close to torch
    autograd's (A) as the same network in another fp32 summation order does (B), window by window, factor 4; the loss falls by
    10 x; a second run gives the same bits; the weights render."""
    from efficient_nerf_amd import R2LEngine
    from efficient_nerf_amd.generic import GenericR2L
    from efficient_nerf_amd.train import R2LTrainer, learning_rate
    from oracle import r2l_oracle as O
    n, n_batch = 2048, 8
    pool = [_rays(n, 300 + b, 'cuda') for b in range(n_batch)]
    g = torch.Generator().manual_seed(9)
    order = torch.randint(0, n_batch, (N_STEP,), generator=g).tolist()
    t_rands = [torch.rand(n, 16, generator=g).cuda() for _ in range(N_STEP)]
    lrs = [learning_rate(t + 1, 5e-4, 500, '0.0001,100') for t in range(N_STEP)]
    sd0 = O.make_r2l_state(21)
    tr = R2LTrainer(netdepth=88, netwidth=256, use_residual=True, trial=dict(body_arch='resmlp'), max_rays=n)

    def run_hip():
        tr.load_state_dict(sd0)
        tr.load_optimizer_state_dict({'state': {}, 'param_groups': tr.optimizer_state_dict()['param_groups']})
        losses = []
        for t in range(N_STEP):
            ro, rd, tgt = pool[order[t]]
            loss, _ = tr.step(ro, rd, tgt, lrs[t], 1., t_rands[t])
            losses.append(loss.clone())
        return torch.cat(losses).cpu(), tr.state_dict()

    H1, sd_h = run_hip()
    H2, sd_h2 = run_hip()
    assert torch.equal(H1, H2) and all(torch.equal(sd_h[k], sd_h2[k]) for k in sd_h)       # bit-identical from run to run

    def run_torch(sd):
        prm = {k: v.detach().cuda().clone().requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.Adam(list(prm.values()), lr=1.0, betas=(0.9, 0.999))
        losses = []
        for t in range(N_STEP):
            ro, rd, tgt = pool[order[t]]
            emb = tr.embed(ro, rd, 1., t_rands[t]).clone()
            for gp in opt.param_groups:
                gp['lr'] = lrs[t]
            loss = ((O.r2l_forward(prm, emb) - tgt) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach().reshape(1))
        return torch.cat(losses).cpu()

    A, B = run_torch(sd0), run_torch(_permute_blocks(sd0))
    H, A, B = H1.double(), A.double(), B.double()
    print(f'first loss {A[0]:.6f}; mean of steps 50-99: HIP {H[50:].mean():.6f}, A {A[50:].mean():.6f} (1/{A[0] / A[50:].mean():.0f})')
    band = 0.
    rows = []
    for a, b in WINDOWS:
        d_h = float(((H[a:b] - A[a:b]).abs() / A[a:b]).max())
        d_b = float(((B[a:b] - A[a:b]).abs() / A[a:b]).max())
        band = max(band, d_b)
        rows.append((a, b, d_h, d_b, band))
        print(f'steps [{a}, {b}): d(HIP) = {d_h:.2e}, d(B) = {d_b:.2e}, band so far {band:.2e}')
    for a, b, d_h, d_b, bnd in rows:
        assert d_h <= 4 * bnd, (a, b, d_h, bnd)
    assert float(H[50:].mean()) < float(H[0]) / 10
    # the trained weights render on the fused engine and on the generic path
    H_img = 32
    focal = O.focal_from_angle(H_img)
    c2w = O.pose_spherical(30., -30., 4.)
    eng = R2LEngine(H_img, H_img, focal, n_block=43).load_state_dict(sd_h)
    rgb = eng.render(c2w)
    gen = GenericR2L(H_img, H_img, focal, netdepth=88, netwidth=256, trial=dict(body_arch='resmlp')).load_state_dict(sd_h)
    rgb_g = gen.render(c2w)
    eng.close()
    assert rgb.shape == rgb_g.shape == (H_img * H_img, 3) and torch.isfinite(rgb).all()
    assert float((rgb - rgb_g).abs().max()) < 1e-4


# ---- 6. optimizer state interchange ------------------------------------------------------------------------------------------
def test_optimizer_state_interchange_with_torch_adam(pkg):
    """three HIP steps, the state into torch.optim.Adam, one given gradient applied in both: as close as Adam alone (test 2)"""
    from efficient_nerf_amd.train import R2LTrainer
    from oracle import r2l_oracle as O
    n = 300
    trial = dict(body_arch='resmlp', n_learnable=2)
    tr = R2LTrainer(n_sample=4, L=3, netdepth=6, netwidth=64, use_residual=True, trial=trial, max_rays=n)
    tr.load_state_dict(O.make_v3_2_state(4, 6, 64, tr.input_dim, '', 'relu', trial))
    ro, rd, tgt = _rays(n, 8, 'cuda')
    for k in range(3):
        tr.step(ro, rd, tgt, 1e-3 * (k + 1))
    osd, sd = tr.optimizer_state_dict(), tr.state_dict()
    assert sorted(osd['state']) == list(range(len(sd))) and all(float(s['step']) == 3 for s in osd['state'].values())
    g = torch.Generator().manual_seed(3)
    given = {k: torch.randn(v.shape, generator=g) * 10 ** (-6 * torch.rand(v.shape, generator=g)) for k, v in sd.items()}
    lr = 7e-4
    outs = {}
    for dtype in (torch.float64, torch.float32):
        prm = [torch.nn.Parameter(v.to(dtype).clone()) for v in sd.values()]          # model.parameters() order
        opt = torch.optim.Adam(prm, lr=1.0, betas=(0.9, 0.999))
        opt.load_state_dict(tr.optimizer_state_dict())          # a fresh copy: torch steps the `step` tensors it is given in place
        assert opt.param_groups[0]['lr'] == 3e-3
        opt.param_groups[0]['lr'] = lr
        for p_, k in zip(prm, sd):
            p_.grad = given[k].to(dtype)
        opt.step()
        outs[dtype] = {k: p_.detach() for p_, k in zip(prm, sd)}
        if dtype == torch.float32:                                                    # and back: torch's state resumes here
            tr2 = R2LTrainer(n_sample=4, L=3, netdepth=6, netwidth=64, use_residual=True, trial=trial, max_rays=n)
            tr2.load_state_dict(outs[dtype]).load_optimizer_state_dict(opt.state_dict())
            assert tr2.t == 4 and all(torch.equal(tr2.exp_avg[k].cpu(), opt.state[p_]['exp_avg']) for p_, k in zip(prm, sd))
    for k, v in given.items():
        tr.g[k].copy_(v)
    tr.adam(lr)
    hip = tr.state_dict()
    gap_hip = max(float((hip[k].double() - outs[torch.float64][k]).abs().max()) for k in sd)
    gap_t32 = max(float((outs[torch.float32][k].double() - outs[torch.float64][k]).abs().max()) for k in sd)
    print(f'state interchange: max|p_hip - p_f64| = {gap_hip:.3e}, max|p_torch_fp32 - p_f64| = {gap_t32:.3e}')
    assert gap_hip <= 4 * gap_t32


# ---- 7. command line ---------------------------------------------------------------------------------------------------------
def test_cli_trains_and_the_checkpoint_renders(pkg, tmp_path):
    """main.py with the README's flags as a child process on a few synthetic shards, then --render_only on what it wrote"""
    import re
    data = tmp_path / 'shards'
    data.mkdir()
    for k in range(4):
        o, d, tgt = _rays(512, 400 + k)
        np.save(str(data / f'pseudo_{k}.npy'), torch.cat([o, d, tgt], -1).numpy().astype(np.float32))
    base = ['--model_name', 'R2L', '--config', os.path.join(ROOT, 'configs', 'lego_noview.txt'), '--n_sample_per_ray', '16', '--netwidth', '256',
            '--netdepth', '88', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp', '--basedir', str(tmp_path), '--expname', 'cli']
    cmd = ['timeout', '-k', '10', '240', sys.executable, os.path.join(ROOT, 'main.py')] + base + [
        '--datadir_kd', str(data), '--N_iters', '20', '--N_rand', '2', '--data_mode', 'rays', '--hard_ratio', '0.2', '--hard_mul', '2',
        '--warmup_lr', '0.0001,200', '--i_weights', '10', '--i_print', '5']
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('[TRAIN] Iter')]
    assert len(lines) == 4, r.stdout[-3000:]
    hist = [float(re.search(r'hist_psnr (\S+)', ln).group(1)) for ln in lines]
    assert all(re.search(r'psnr \S+ hist_psnr \S+ LR \d\.\d{10}', ln) for ln in lines)
    assert hist[-1] > hist[0], hist                       # the smoothed loss falls
    tars = [f for f in os.listdir(tmp_path / 'cli' / 'weights') if f.endswith('.tar')]
    assert tars, os.listdir(tmp_path / 'cli')
    ck = str(tmp_path / 'cli' / 'weights' / tars[0])
    saved = torch.load(ck, map_location='cpu', weights_only=False)
    assert saved['global_step'] == 20 and len(saved['optimizer_state_dict']['state']) == 2 * 88 and 'head.0.weight' in saved['network_fn_state_dict']
    out = str(tmp_path / 'render')
    cmd = ['timeout', '-k', '10', '240', sys.executable, os.path.join(ROOT, 'main.py')] + base + [
        '--pretrained_ckpt', ck, '--render_only', '--synthetic_poses', '1', '--H', '32', '--precision', 'auto', '--outdir', out]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rgbs = np.load(os.path.join(out, 'rgbs.npy'))
    assert rgbs.shape[-1] == 3 and np.isfinite(rgbs).all()

"""Training of the NeRF teacher (main.py:1136-1513 with --model_name nerf, --data_mode images: no_batching on Blender scenes,
use_batching on LLFF scenes; the step is render_rays, main.py:624-756, under autograd plus torch.optim.Adam): both networks'
forward and backward passes, both volume-rendering scans and their backward pass, the two rgb losses and Adam as launches of the
library's fp32 kernels (csrc/r2l_generic.hip, r2l_train.hip, nerf_kernels.hip, nerf_train.hip; include/r2l_hip.h).  On LLFF a
step's rays come from the image bytes in one launch (RayBatches, nerf_train_batch_rays).

NeRFTrainer holds the coarse network's parameters, then the fine one's, in one flat device buffer (flat_trainer.FlatAdam), and the
saved output of every layer of both passes for the backward pass.  torch supplies the buffers, the stream and the random draws
(t_rand, u, the density noise); every number of a step is computed by the library in exact fp32, and a step is bit-identical from
run to run (no float atomics anywhere).

The networks are generic.nerf_plan's: every pair create_nerf builds (main.py:407-453).  The reference's two torch.cat inputs are
column slices of wider buffers, as in generic._NeRFNet.forward.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from ._lib import R2LError, check, current_stream, dptr, lib
from .flat_trainer import ACT_NONE, ACT_RELU, FlatAdam, init_linears
from .generic import _strip, _view, nerf_plan
from .train import jitter_z_vals, pair_networks, refuse_negative_i_testset, run_iterations

SKIPS = (4,)
PREFIXES = ('network_fn', 'network_fine')


def reference_order(D, W, input_ch, input_ch_views, output_ch, use_viewdirs):
    """(key, in_dim, out_dim) of one NeRF in the order its constructor creates the modules (model/nerf_raybased.py:357-375), which
    is model.parameters() order and so the optimizer's: pts_linears.*, views_linears.0 (always built), then feature_linear,
    alpha_linear, rgb_linear -- or output_linear.  generic.nerf_plan lists the same layers in execution order."""
    plan = {k: (i, o) for k, i, o in nerf_plan(D, W, input_ch, input_ch_views, output_ch, SKIPS, use_viewdirs)}
    keys = [f'pts_linears.{i}' for i in range(D)] + ['views_linears.0']
    keys += ['feature_linear', 'alpha_linear', 'rgb_linear'] if use_viewdirs else ['output_linear']
    plan.setdefault('views_linears.0', (input_ch_views + W, W // 2))
    return [(k,) + plan[k] for k in keys]


class _Net:
    """Shapes and per-step buffers of one of the two networks"""

    def __init__(self, prefix, D, W, S):
        self.prefix, self.D, self.W, self.S = prefix, D, W, S


class NeRFTrainer(FlatAdam):
    """render_rays (main.py:624-756) of a batch of rays + img2mse(rgb) + img2mse(rgb0) + their gradients + torch.optim.Adam(betas
    (0.9, 0.999)) over list(model.parameters()) + list(model_fine.parameters()) (main.py:425-445), on the device.

    Parameter names carry the network's checkpoint key: network_fn.pts_linears.0.weight, ..., network_fine.rgb_linear.bias.
    Without use_viewdirs the reference still builds views_linears.0 and never calls it: it is in the state dict, its gradient stays
    zero and Adam leaves it as it is (FlatAdam._frozen); the saved optimizer state has no entry under its two indices, as torch's
    has none for a parameter whose .grad is None, and a state with or without such entries loads.

    max_rays: the largest batch a step may carry (the buffers are allocated once, at load_state_dicts)."""
    _min_rays = 1

    def __init__(self, near=2., far=6., N_samples=64, N_importance=128, multires=10, multires_views=4, i_embed=0, netdepth=8,
                 netwidth=256, netdepth_fine=8, netwidth_fine=256, use_viewdirs=True, white_bkgd=False, lindisp=False,
                 max_rays=1024, device=None):
        self._set_device(device, max_rays)
        self.near, self.far = float(near), float(far)
        self.N_samples, self.N_importance = int(N_samples), int(N_importance)
        self.multires, self.multires_views, self.i_embed = int(multires), int(multires_views), int(i_embed)
        if self.i_embed not in (0, -1):
            raise R2LError(f'i_embed={i_embed}: 0 (positional encoding) or -1 (none), utils/run_nerf_raybased_helpers.py:59-74')
        if self.N_samples < 1 or self.N_importance < 0 or (self.N_importance > 0 and not 3 <= self.N_samples <= 65):
            raise R2LError(f'N_samples={N_samples} N_importance={N_importance}: sample_pdf takes 2 .. 64 bins (N_samples - 1 of them)')
        self.use_viewdirs, self.white_bkgd, self.lindisp = bool(use_viewdirs), bool(white_bkgd), bool(lindisp)
        self.input_ch = 3 if self.i_embed == -1 else 3 * (2 * self.multires + 1)
        self.input_ch_views = 0 if not self.use_viewdirs else (3 if self.i_embed == -1 else 3 * (2 * self.multires_views + 1))
        self.output_ch = 5 if self.N_importance > 0 else 4          # main.py:426
        self.raw_ch = 4 if self.use_viewdirs else self.output_ch
        self.nets = [_Net(PREFIXES[0], int(netdepth), int(netwidth), self.N_samples)]
        if self.N_importance > 0:
            self.nets.append(_Net(PREFIXES[1], int(netdepth_fine), int(netwidth_fine), self.N_samples + self.N_importance))
        for net in self.nets:
            if net.D < 1 or net.W < 2:
                raise R2LError(f'{net.prefix}: netdepth {net.D} netwidth {net.W}')
            if (net.D - 1) in SKIPS:
                raise R2LError(f'{net.prefix}: netdepth {net.D} makes the last pts_linears layer a skip layer: alpha_linear / feature_linear '
                               f'take W inputs (the reference fails too)')
            net.layers = OrderedDict((k, (i, o)) for k, i, o in reference_order(net.D, net.W, self.input_ch, self.input_ch_views,
                                                                                 self.output_ch, self.use_viewdirs))
        # main.py:676-682 on the host as the reference's first ray computes it (near, far are the same for every ray)
        t = torch.linspace(0., 1., steps=self.N_samples)
        nr, fr = torch.tensor([self.near]), torch.tensor([self.far])
        z = nr * (1. - t) + fr * t if not self.lindisp else 1. / (1. / nr * (1. - t) + 1. / fr * t)
        self.z_coarse = z.to(torch.float32).contiguous()
        # flat layout: the coarse network, then the fine one; module by module in creation order
        self._set_layout([(f'{net.prefix}.{k}', i, o) for net in self.nets for k, (i, o) in net.layers.items()])
        if not self.use_viewdirs:
            self._frozen = frozenset(f'{net.prefix}.views_linears.0.{kind}' for net in self.nets for kind in ('weight', 'bias'))
        self.last = {}

    # ---- state -------------------------------------------------------------------------------------------------------------
    @property
    def flops_per_ray(self):
        """of the two forward passes; a training step is about three times that (g_x and g_W cost one forward each)"""
        return 2 * sum(net.S * sum(i * o for k, (i, o) in net.layers.items() if self.use_viewdirs or k != 'views_linears.0')
                       for net in self.nets)

    def _per_point_floats(self, net):
        """saved layer outputs and inputs of one point of one network"""
        ic, icv, W = self.input_ch, self.input_ch_views, net.W
        return 3 + (ic + W) + (W + icv + W // 2 if self.use_viewdirs else 0) + W * sum(1 for i in range(net.D) if i not in SKIPS) + self.raw_ch + 4

    def activation_bytes(self, n=None):
        n = self.max_rays if n is None else n
        return 4 * n * sum(net.S * self._per_point_floats(net) for net in self.nets)

    def _allocate(self):
        n, dev = self.max_rays, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        ic, icv = self.input_ch, self.input_ch_views
        m_max = n * max(net.S for net in self.nets)
        w_max = max(net.W for net in self.nets)
        slabs = lib().r2l_train_grad_weight_slabs(m_max)
        ws_floats = max(1, slabs * max(i * o + o for net in self.nets for i, o in net.layers.values()))
        grad_floats = m_max * (2 * (ic + w_max) + w_max + (w_max + icv + w_max) + 4 + self.raw_ch)
        want = self.activation_bytes() + 4 * (4 * self.n_param + grad_floats + ws_floats)
        sizes = (f'about {want / 2 ** 30:.1f} GiB (saved layer outputs {self.activation_bytes() / 2 ** 30:.1f} GiB: ' +
                 ', '.join(f'{net.prefix} {n * net.S} points x {self._per_point_floats(net)} floats' for net in self.nets) +
                 f'; gradient buffers {4 * grad_floats / 2 ** 30:.1f} GiB; slab workspace {4 * ws_floats / 2 ** 30:.2f} GiB)')
        free = torch.cuda.mem_get_info(dev)[0]
        if want > free:               # before anything is allocated: a step that cannot fit leaves the device as it found it
            raise R2LError(f'the training buffers for {n} rays per step need {sizes}; the device has {free / 2 ** 30:.1f} GiB free. '
                           f'Lower --N_rand.')
        try:
            with torch.cuda.device(dev):
                self._allocate_flat()
                for net in self.nets:
                    m, W = n * net.S, net.W
                    net.pts = torch.empty((m, 3), **f32)
                    net.cat = torch.empty((m, ic + W), **f32)
                    net.views = torch.empty((m, W + icv), **f32) if self.use_viewdirs else None
                    net.hv = torch.empty((m, W // 2), **f32) if self.use_viewdirs else None
                    net.acts = [None if i in SKIPS else torch.empty((m, W), **f32) for i in range(net.D)]
                    net.raw = torch.empty((m, self.raw_ch), **f32)
                    net.raw4 = net.raw if self.raw_ch == 4 else torch.empty((m, 4), **f32)
                    net.rgb = torch.empty((n, 3), **f32)
                    net.g_rgb = torch.empty((n, 3), **f32)
                    net.loss = torch.zeros((1,), **f32)
                # gradient work buffers, shared by the two backward passes (they run one after the other on one stream)
                self._GA, self._GB = (torch.empty((m_max * (ic + w_max),), **f32) for _ in range(2))
                self._Z = torch.empty((m_max * w_max,), **f32)
                self._gviews = torch.empty((m_max * (w_max + icv),), **f32) if self.use_viewdirs else None
                self._ghv, self._gzv = ((torch.empty((m_max * (w_max // 2),), **f32) for _ in range(2)) if self.use_viewdirs else (None, None))
                self._g_raw = torch.empty((m_max * 4,), **f32)
                self._g_out = torch.zeros((m_max * self.raw_ch,), **f32) if self.raw_ch != 4 else None
                self._err = torch.empty((n,), **f32)
                self._ws = torch.empty((ws_floats,), **f32)
                self._loss_ws = torch.empty(((n + 255) // 256,), **f32)
                self._scan = [torch.empty((n,), **f32) for _ in range(3)]              # disp, acc, depth: computed, not trained on
                self._weights = torch.empty((n, self.N_samples), **f32)
                self._z_dev = self.z_coarse.to(dev)
        except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
            self._release_flat()
            for net in self.nets:
                net.__dict__ = {k: v for k, v in net.__dict__.items() if not torch.is_tensor(v) and k != 'acts'}
            raise R2LError(f'cannot allocate the training buffers for {n} rays per step: {sizes}: {e}. Lower --N_rand.') from e

    def init_state_dicts(self, seed=None):
        """nn.Linear's default initialisation of every module, in creation order: (coarse, fine or None)"""
        sd = init_linears([(name, i, o) for name, (i, o) in self._dims.items()], seed)
        return self._split(sd, lambda v: v)

    def load_state_dicts(self, network_fn_state_dict, network_fine_state_dict=None):
        sds = [_strip(network_fn_state_dict)]
        if self.N_importance > 0:
            if network_fine_state_dict is None:
                raise R2LError('N_importance > 0 needs network_fine_state_dict (main.py:436-445)')
            sds.append(_strip(network_fine_state_dict))
        for net, sd in zip(self.nets, sds):
            for k, (i, o) in net.layers.items():
                for kind, shape in (('weight', (o, i)), ('bias', (o,))):
                    if f'{k}.{kind}' not in sd:
                        raise R2LError(f'{net.prefix}_state_dict lacks {k}.{kind} (has e.g. {sorted(sd)[:4]})')
                    if tuple(sd[f'{k}.{kind}'].shape) != shape:
                        raise R2LError(f'{net.prefix}: {k}.{kind} is {tuple(sd[f"{k}.{kind}"].shape)}, the flags describe {shape}')
        if self._param is None:
            self._allocate()
        for net, sd in zip(self.nets, sds):
            for k in net.layers:
                for kind in ('weight', 'bias'):
                    self.p[f'{net.prefix}.{k}.{kind}'].copy_(torch.as_tensor(sd[f'{k}.{kind}']).detach().to(torch.float32))
        return self

    def _split(self, named, copy):
        """an OrderedDict keyed by parameter name as (coarse, fine or None) without the networks' prefixes"""
        out = []
        for net in self.nets:
            cut = len(net.prefix) + 1
            out.append(OrderedDict((k[cut:], copy(v)) for k, v in named.items() if k.startswith(net.prefix + '.')))
        return out[0], (out[1] if len(out) > 1 else None)

    def state_dicts(self):
        """(network_fn_state_dict, network_fine_state_dict or None) on the host, keyed as the reference's checkpoint"""
        self._need_state()
        return self._split(self.p, lambda v: v.detach().cpu().clone())

    def grads(self):
        """the gradients of the last forward_backward, as state_dicts() is keyed: (coarse, fine or None), on the device"""
        self._need_state()
        return self._split(self.g, lambda v: v.detach().clone())

    def checkpoint_networks(self):
        return pair_networks(*self.state_dicts())

    # ---- launches beside FlatAdam's ----------------------------------------------------------------------------------------
    def _embed(self, x, L, out):
        """get_embedder(L, i_embed) of x [m, 3] into the view `out`"""
        if self.i_embed == -1:
            out.copy_(x)
            return
        op, ldo = _view(out)
        check(lib().nerf_embed(dptr(x), 3, x.shape[0], 3, L, op, ldo, current_stream()))

    def _layer_io(self, net, m):
        """per pts_linears layer: (input view, output view) over the first m points"""
        ic = self.input_ch
        cat = net.cat[:m]
        io, x = [], cat[:, :ic]
        for i in range(net.D):
            y = cat[:, ic:] if i in SKIPS else net.acts[i][:m]
            io.append((x, y))
            x = cat if i in SKIPS else y
        return io

    def _net_forward(self, net, ro, rd, viewdirs, z):
        """network_query_fn(rays_o + rays_d * z, viewdirs, network) (main.py:65-87, 701-707) keeping every layer's output:
        raw [n * S, raw_ch] (a view)"""
        n, S, W, ic, pre = ro.shape[0], net.S, net.W, self.input_ch, net.prefix + '.'
        m = n * S
        pts, cat, raw = net.pts[:m], net.cat[:m], net.raw[:m]
        check(lib().r2l_sample_points(dptr(ro), dptr(rd), n, dptr(z), S, 1, dptr(pts), current_stream()))
        self._embed(pts, self.multires, cat[:, :ic])
        io = self._layer_io(net, m)
        for i, (x, y) in enumerate(io):
            self._linear(f'{pre}pts_linears.{i}', x, y, ACT_RELU)
        h = io[-1][1]
        if not self.use_viewdirs:
            self._linear(pre + 'output_linear', h, raw, ACT_NONE)
            return raw
        views, hv = net.views[:m], net.hv[:m]
        dirs = viewdirs[:, None, :].expand(n, S, 3).reshape(m, 3).contiguous()        # main.py:76-77
        self._embed(dirs, self.multires_views, views[:, W:])
        self._linear(pre + 'alpha_linear', h, raw[:, 3:4], ACT_NONE)
        self._linear(pre + 'feature_linear', h, views[:, :W], ACT_NONE)
        self._linear(pre + 'views_linears.0', views, hv, ACT_RELU)
        self._linear(pre + 'rgb_linear', hv, raw[:, :3], ACT_NONE)
        return raw

    def _scan_forward(self, net, raw, z, rd, noise, weights):
        """raw2outputs (main.py:556-621): rgb_map into net.rgb; returns the [n, S, 4] block the scan read"""
        n, S = rd.shape[0], net.S
        raw4 = net.raw4[:n * S]
        if raw4.data_ptr() != raw.data_ptr():
            raw4.copy_(raw[:, :4])                    # raw2outputs reads channels 0..3 (main.py:588-600); the fifth is never used
        disp, acc, depth = (b[:n] for b in self._scan)
        check(lib().nerf_raw2outputs_noise(dptr(raw4), dptr(z), dptr(rd), dptr(noise), n, S, int(self.white_bkgd), dptr(net.rgb[:n]),
                                           dptr(disp), dptr(acc), dptr(weights), dptr(depth), current_stream()))
        return raw4

    def _scan_backward(self, net, raw4, z, rd, noise, g_raw):
        """g_raw [n * S, 4] from net.g_rgb (csrc/nerf_train.hip)"""
        n = rd.shape[0]
        check(lib().nerf_train_raw2outputs_backward(dptr(raw4), dptr(z), dptr(rd), dptr(noise), n, net.S, int(self.white_bkgd),
                                                    dptr(net.g_rgb[:n]), dptr(g_raw), current_stream()))
        return g_raw

    def _net_backward(self, net, raw4, z, rd, noise, n):
        """from net.g_rgb (the loss's gradient at rgb_map) through the scan and the network into the flat gradient buffer"""
        S, W, ic, pre = net.S, net.W, self.input_ch, net.prefix + '.'
        m = n * S
        mat = lambda flat, cols: flat[:m * cols].view(m, cols)
        g_raw = self._scan_backward(net, raw4, z, rd, noise, mat(self._g_raw, 4))
        io = self._layer_io(net, m)
        h = io[-1][1]
        g_h = mat(self._GA, W)
        if self.use_viewdirs:
            views, hv = net.views[:m], net.hv[:m]
            g_hv, g_zv, g_views = mat(self._ghv, W // 2), mat(self._gzv, W // 2), mat(self._gviews, W + self.input_ch_views)
            self._grad_weight(pre + 'rgb_linear', g_raw[:, :3], hv)
            self._grad_input(pre + 'rgb_linear', g_raw[:, :3], g_hv, False)
            self._act_backward(pre + 'views_linears.0', g_hv, hv, g_zv)
            self._grad_weight(pre + 'views_linears.0', g_zv, views)
            self._grad_input(pre + 'views_linears.0', g_zv, g_views, False)
            self._grad_weight(pre + 'feature_linear', g_views[:, :W], h)
            self._grad_input(pre + 'feature_linear', g_views[:, :W], g_h, False)
            self._grad_weight(pre + 'alpha_linear', g_raw[:, 3:4], h)             # alpha and feature both read h: their g_h add up
            self._grad_input(pre + 'alpha_linear', g_raw[:, 3:4], g_h, True)
        else:
            g_out = g_raw
            if self.raw_ch != 4:                      # the unused fifth output: its column of g_out stays zero
                g_out = mat(self._g_out, self.raw_ch)
                g_out[:, :4].copy_(g_raw)
            self._grad_weight(pre + 'output_linear', g_out, h)
            self._grad_input(pre + 'output_linear', g_out, g_h, False)
        g_y, cur, other = g_h, self._GA, self._GB
        g_z = mat(self._Z, W)
        for i in range(net.D - 1, -1, -1):
            x, y = io[i]
            self._act_backward(f'{pre}pts_linears.{i}', g_y, y, g_z)
            self._grad_weight(f'{pre}pts_linears.{i}', g_z, x)
            if i > 0:                                 # the embedding has no parameters: no g_x for layer 0
                g_x = mat(other, x.shape[1])
                self._grad_input(f'{pre}pts_linears.{i}', g_z, g_x, False)
                g_y = g_x[:, ic:] if (i - 1) in SKIPS else g_x     # behind a skip layer x = [input_pts | h]
                cur, other = other, cur

    # ---- one step ----------------------------------------------------------------------------------------------------------
    def _draw(self, given, shape, what, scale=None):
        if given is None:
            t = torch.rand(shape, dtype=torch.float32, device=self.device) if scale is None else \
                torch.randn(shape, dtype=torch.float32, device=self.device) * scale
            return t
        t = given.to(self.device, torch.float32).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise R2LError(f'{what} is {tuple(t.shape)}, expected {tuple(shape)}')
        return t

    def forward_backward(self, rays_o, rays_d, target, perturb=1., raw_noise_std=0., t_rand=None, u=None, noise=None, viewdirs=None):
        """loss = img2mse(rgb, target) + img2mse(rgb0, target) (a one-element device tensor; the coarse term alone with
        N_importance = 0); the gradients are left in the flat buffer (grads()).

        t_rand [n, N_samples], u [n, N_importance] in [0, 1) and noise = (noise0 [n, N_samples], noise1 [n, N_samples +
        N_importance]) (what is added to the density in front of its relu: randn * raw_noise_std) replace the draws of main.py:691,
        helpers:298-307 and main.py:592-598; by default they are torch draws on the device.  self.last keeps the step's detached
        quantities: per pass the embedded inputs (`emb0`, `emb1`: [n * S, input_ch]; `dirs0`, `dirs1`: the embedded view
        directions), the depths (`z0`, `z1`), the noise, `raw0` / `raw1`, and `rgb0` / `rgb`.

        viewdirs [n, 3]: unit view directions used in place of rays_d / ||rays_d|| -- those of the world-space rays when rays_o /
        rays_d are their NDC projection (main.py:148-162); rays_o / rays_d are sampled and composited along as they are."""
        from .teacher import merge_sorted, sample_pdf
        self._need_state()
        n = rays_o.shape[0]
        dev = self.device
        ro, rd, tgt = self._on_device(n, rays_o=rays_o, rays_d=rays_d, target=target)
        given_dirs = self._on_device(n, viewdirs=viewdirs)[0] if viewdirs is not None and self.use_viewdirs else None
        S0, Ni = self.N_samples, self.N_importance
        fine = Ni > 0
        noises = [None, None]
        if noise is not None or raw_noise_std > 0.:
            given = noise if noise is not None else (None, None)
            noises = [self._draw(given[k], (n, net.S), f'noise[{k}]', raw_noise_std) for k, net in enumerate(self.nets)]
        with torch.cuda.device(dev):
            viewdirs = given_dirs
            if viewdirs is None and self.use_viewdirs:
                viewdirs = rd / torch.norm(rd, dim=-1, keepdim=True)                                  # main.py:148-157
            if perturb > 0.:
                z0 = jitter_z_vals(self._z_dev, n, self._draw(t_rand, (n, S0), 't_rand'))             # main.py:684-699
            else:
                z0 = self._z_dev.expand(n, S0).contiguous()
            c, f = self.nets[0], (self.nets[1] if fine else None)
            weights = self._weights[:n]
            raw0 = self._net_forward(c, ro, rd, viewdirs, z0)
            raw0_4 = self._scan_forward(c, raw0, z0, rd, noises[0], weights)
            self.last = dict(z0=z0, raw0=raw0, rgb0=c.rgb[:n], noise0=noises[0], emb0=c.cat[:n * S0, :self.input_ch],
                             dirs0=c.views[:n * S0, c.W:] if self.use_viewdirs else None)
            if fine:
                z_mid = .5 * (z0[:, 1:] + z0[:, :-1])                                                 # main.py:722-732
                z_samples = sample_pdf(z_mid, weights[:, 1:-1], Ni, det=(perturb == 0.),
                                       u=None if perturb == 0. else self._draw(u, (n, Ni), 'u'))
                if perturb > 0.:          # drawn u: the samples come out in u's order, and main.py:730-732 is a real sort
                    z_samples = torch.sort(z_samples, -1)[0]
                z1 = merge_sorted(z0, z_samples)
                raw1 = self._net_forward(f, ro, rd, viewdirs, z1)
                raw1_4 = self._scan_forward(f, raw1, z1, rd, noises[1], None)
                self.last.update(z1=z1, z_samples=z_samples, raw1=raw1, rgb=f.rgb[:n], noise1=noises[1],
                                 emb1=f.cat[:n * f.S, :self.input_ch], dirs1=f.views[:n * f.S, f.W:] if self.use_viewdirs else None)
            else:
                self.last['rgb'] = c.rgb[:n]
            top = f if fine else c
            for net in self.nets:                     # img2mse and its gradient at rgb_map; the per-ray error of the final rgb
                self._mse_loss(net.rgb[:n], tgt, 0, net.g_rgb[:n], net.loss, self._err[:n] if net is top else None)
            if fine:
                self._net_backward(f, raw1_4, z1, rd, noises[1], n)
            self._net_backward(c, raw0_4, z0, rd, noises[0], n)
            self.loss_rgb = top.loss
            return c.loss + f.loss if fine else c.loss                                                 # main.py:1362-1380

    def step(self, rays_o, rays_d, target, lr, perturb=1., raw_noise_std=0., t_rand=None, u=None, noise=None, viewdirs=None):
        """forward_backward + Adam.  Returns (loss [1], loss_rgb [1]): the sum the gradients are of, and img2mse of the final rgb
        alone (what the reference's psnr line reports, main.py:1377-1379)."""
        loss = self.forward_backward(rays_o, rays_d, target, perturb, raw_noise_std, t_rand, u, noise, viewdirs)
        self.adam(lr)
        return loss, self.loss_rgb


# ---------------------------------------------------------------------------------------------------------------------------
# the loop of main.py:1136-1513 for --model_name nerf, --data_mode images: no_batching on Blender, use_batching on LLFF
# ---------------------------------------------------------------------------------------------------------------------------
class RayBatches:
    """The reference's use_batching loop (main.py:1141-1162, 1199-1210) without its bank rays_rgb [n, 3, 3]: row r of the bank is a
    function of the image bytes, the poses and r, so the bytes [n_img, H, W, 3], the poses [n_img, 3, 4] and the order of the rows (an
    int64 permutation of n = n_img * H * W, image-major, then row, then column) are what is kept on the device, and a step's rows
    are computed by one launch (nerf_train_batch_rays).

    The order follows the reference draw for draw: np.random.permutation(n) of the global numpy stream first (np.random.shuffle of
    an [n, 3, 3] array walks the same Fisher-Yates over its first axis: the same draws, the same order), then after every epoch
    perm = perm[torch.randperm(n)] from torch's CPU default generator.  A batch is the window [i_batch, i_batch + N_rand) cut at n:
    the last batch of an epoch is short.  A resumed run starts a new epoch from a fresh draw (nothing of this is in a checkpoint).

    near: ndc_rays' near plane (1 in the reference, main.py:162) when ndc."""

    def __init__(self, image_bytes, poses, focal, N_rand, ndc, near=1., device=None, log=print):
        image_bytes = torch.as_tensor(image_bytes)
        if image_bytes.dtype != torch.uint8 or image_bytes.dim() != 4 or image_bytes.shape[-1] != 3:
            raise R2LError(f'image bytes are {image_bytes.dtype} {tuple(image_bytes.shape)}, expected uint8 [n_img, H, W, 3]')
        poses = torch.as_tensor(poses, dtype=torch.float32)[:, :3, :4]
        self.n_img, self.H, self.W = (int(v) for v in image_bytes.shape[:3])
        if tuple(poses.shape) != (self.n_img, 3, 4):
            raise R2LError(f'poses are {tuple(poses.shape)} for {self.n_img} images')
        self.focal, self.N_rand, self.ndc, self.near, self.log = float(focal), int(N_rand), bool(ndc), float(near), log
        if self.N_rand < 1:
            raise R2LError(f'N_rand {N_rand}')
        self.n = self.n_img * self.H * self.W
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._upload(image_bytes.contiguous(), poses.contiguous())
        self.perm = torch.from_numpy(np.random.permutation(self.n).astype(np.int64))      # main.py:1156
        self._set_order()
        self.i_batch = 0

    # the three places that touch the device (a test replaces them to follow the index stream on the host)
    def _upload(self, image_bytes, poses):
        self._bytes, self._poses = image_bytes.to(self.device), poses.to(self.device)

    def _set_order(self):
        self._order = self.perm.to(self.device)

    def _launch(self, begin, rows):
        f32 = dict(dtype=torch.float32, device=self.device)
        out = torch.empty((4, rows, 3), **f32)
        order = self._order[begin:begin + rows]             # a view: the permutation offset to the step's window
        with torch.cuda.device(self.device):
            check(lib().nerf_train_batch_rays(self._bytes.data_ptr(), self.n_img, self.H, self.W, dptr(self._poses), self.focal,
                                              order.data_ptr(), rows, int(self.ndc), self.near, dptr(out[0]), dptr(out[1]), dptr(out[2]),
                                              dptr(out[3]), current_stream()))
        return out[0], out[1], out[2], out[3]

    def next(self):
        """(rays_o, rays_d, viewdirs, target) of the next step, each [rows, 3] on the device; rows = N_rand, fewer in an epoch's
        last batch"""
        begin = self.i_batch
        rows = min(self.N_rand, self.n - begin)
        batch = self._launch(begin, rows)
        self.i_batch += self.N_rand                           # main.py:1205-1210
        if self.i_batch >= self.n:
            self.log('Shuffle data after an epoch!')
            self.perm = self.perm[torch.randperm(self.n)]
            self._set_order()
            self.i_batch = 0
        return batch


def crop_bounds(H, W, precrop_frac):
    """main.py:1270-1278: the centre crop's (row0, rows, col0, cols)"""
    dH = int(H // 2 * precrop_frac)
    dW = int(W // 2 * precrop_frac)
    return H // 2 - dH, 2 * dH, W // 2 - dW, 2 * dW


def select_coords(H, W, N_rand, crop=None):
    """get_selected_coords(coords, N_rand, 'rand_pixel') (utils/run_nerf_raybased_helpers.py:385-392) over the full image or the
    centre crop of main.py:1270-1287: one np.random.choice(h * w, N_rand, replace=False) of the global numpy stream, row-major
    over the coords grid.  Returns int64 (rows, cols) [N_rand]."""
    r0, h, c0, w = (0, H, 0, W) if crop is None else crop
    if N_rand > h * w:
        raise R2LError(f'N_rand {N_rand} exceeds the {h} x {w} pixels to choose from')
    ix = np.random.choice(h * w, size=[N_rand], replace=False)
    return r0 + ix // w, c0 + ix % w


REFUSALS = {
    'use_batching': 'use_batching (no --no_batching / no_batching = True): teacher training is built for one image per step',
    'llff': '--dataset_type {}: teacher training is built for Blender scenes (--dataset_type blender)',
    'llff_no_batching': '--dataset_type llff: teacher training is built for Blender scenes with no_batching; LLFF scenes train with '
                        'use_batching (no --no_batching / no_batching line, as configs/fern.txt)',
    'rand_patch': '--select_pixel_mode rand_patch: teacher training selects pixels with rand_pixel',
    'i_video': '--i_video {} falls inside this run: the video render is not built for training; pass an --i_video above --N_iters',      # lifted by --write_video
    'datadir_kd': '--datadir_kd with --data_mode images: pseudo images are not built for teacher training',
    'data_mode': '--data_mode {}: the teacher trains on images (--data_mode images)',
    'model_name': '--model_name {}: train_teacher.py trains --model_name nerf (main.py trains the student)',
}


def check_supported(args, start=0):
    """one clear line for each mode of the reference's loop that is not built"""
    if args.model_name != 'nerf':
        raise SystemExit(REFUSALS['model_name'].format(args.model_name))
    if args.dataset_type == 'llff':
        if args.no_batching:
            raise SystemExit(REFUSALS['llff_no_batching'])
    elif not args.no_batching:
        raise SystemExit(REFUSALS['use_batching'])
    elif args.dataset_type != 'blender':
        raise SystemExit(REFUSALS['llff'].format(args.dataset_type))
    if args.select_pixel_mode != 'rand_pixel':
        raise SystemExit(REFUSALS['rand_patch'])
    if args.data_mode != 'images':
        raise SystemExit(REFUSALS['data_mode'].format(args.data_mode))
    if args.datadir_kd:
        raise SystemExit(REFUSALS['datadir_kd'])
    if not getattr(args, 'write_video', False) and args.i_video > 0 and args.N_iters // args.i_video > start // args.i_video:
        raise SystemExit(REFUSALS['i_video'].format(args.i_video))
    refuse_negative_i_testset(args)


def trainer_from_args(args, max_rays, near=2., far=6.):
    """near, far: 2, 6 on Blender (main.py:930-931); on LLFF what llff_split_and_bounds gives"""
    return NeRFTrainer(near, far, N_samples=args.N_samples, N_importance=args.N_importance, multires=args.multires,
                       multires_views=args.multires_views, i_embed=args.i_embed, netdepth=args.netdepth, netwidth=args.netwidth,
                       netdepth_fine=args.netdepth_fine, netwidth_fine=args.netwidth_fine, use_viewdirs=args.use_viewdirs,
                       white_bkgd=args.white_bkgd, lindisp=args.lindisp, max_rays=max_rays)


def test_engine(trainer, args, hwf, near=2., far=6., ndc=False):
    """generic.GenericNeRF at hwf with the trainer's current weights: what the test split and the video are rendered on"""
    from .generic import GenericNeRF
    H, W, focal = hwf
    eng = GenericNeRF(H, W, focal, near, far, N_samples=args.N_samples, N_importance=args.N_importance, multires=args.multires,
                      multires_views=args.multires_views, i_embed=args.i_embed, netdepth=args.netdepth, netwidth=args.netwidth,
                      netdepth_fine=args.netdepth_fine, netwidth_fine=args.netwidth_fine, use_viewdirs=args.use_viewdirs,
                      white_bkgd=args.white_bkgd, lindisp=args.lindisp, ndc=ndc, device=trainer.device)
    eng.load_state_dicts(*trainer.state_dicts())
    return eng


def eval_test_split(trainer, args, hwf, poses, gt, near=2., far=6., ndc=False):
    """render_path over the test split from the current weights (main.py:1442-1456) on generic.GenericNeRF: (test_psnr, test_psnr_v2)"""
    from .frontend import mse2psnr
    H, W, focal = hwf
    eng = test_engine(trainer, args, hwf, near, far, ndc)
    mses = []
    for pose, img in zip(poses, gt):
        rgb = eng.render(pose[:3, :4])['rgb_map'].view(H, W, 3)
        mses.append(float(torch.mean((rgb - img.to(rgb.device)) ** 2).item()))
    return mse2psnr(float(np.mean(mses))), float(np.mean([mse2psnr(m) for m in mses]))


def llff_split_and_bounds(scene, llffhold, no_ndc):
    """main.py:903-919: (i_train, i_val, i_test, near, far) of a loaded LLFF scene.  Every llffhold-th view is held out (llffhold <= 0:
    the loader's own view nearest the average pose), validation is the test set; NDC rays are sampled on [0, 1], world-space rays
    (--no_ndc) from 0.9 x the nearest bound to the farthest."""
    n = len(scene.poses)
    i_test = np.arange(n)[::llffhold] if llffhold > 0 else np.array([scene.i_test])
    i_val = i_test
    i_train = np.array([i for i in np.arange(int(n)) if (i not in i_test and i not in i_val)])
    if no_ndc:
        near, far = float(np.ndarray.min(scene.bds) * .9), float(np.ndarray.max(scene.bds) * 1.)
    else:
        near, far = 0., 1.
    return i_train, i_val, i_test, near, far


def _blender_data(args, start, log):
    """no_batching on a Blender scene (main.py:1212-1292): one training image per step, N_rand of its pixels, the centre crop"""
    from . import blender
    from .frontend import png_reader
    from .teacher import get_rays
    images, poses, hwf, (i_train, i_val, i_test) = blender.load_blender_data(args.datadir, args.half_res, args.testskip, decode=png_reader(args))
    images = blender.composite(images, args.white_bkgd)
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    dev = torch.device('cuda', torch.cuda.current_device())
    crop = crop_bounds(H, W, args.precrop_frac)

    def draw(i):
        img_i = np.random.choice(i_train)                     # main.py:1213
        rays_o, rays_d = get_rays(H, W, focal, poses[img_i, :3, :4], device=dev)
        cropped = i < args.precrop_iters
        if cropped and i == start + 1:
            log(f'[Config] Center cropping of size {crop[1]} x {crop[3]} is enabled until iter {args.precrop_iters}')
        rows, cols = select_coords(H, W, args.N_rand, crop if cropped else None)
        rows, cols = torch.as_tensor(rows, device=dev), torch.as_tensor(cols, device=dev)
        return rays_o[rows, cols], rays_d[rows, cols], images[img_i].to(dev)[rows, cols]

    loaded = (f'Loaded blender {tuple(images.shape)} from "{args.datadir}": {len(i_train)} train / {len(i_val)} val / {len(i_test)} test '
              f'images, {H} x {W}, focal {focal:.4f}')
    return dict(hwf=(H, W, focal), bounds=(2., 6.), ndc=False, max_rays=args.N_rand, draw=draw, step_args={}, loaded=loaded,    # main.py:930-931
                test=(poses[i_test], images[i_test]))


def _llff_data(args, log):
    """use_batching on an LLFF scene (main.py:890-919, 1137-1162, 1199-1210): random rays over all training images, no centre crop;
    NDC unless --no_ndc"""
    from . import llff
    from .frontend import png_reader
    try:
        scene = llff.load_scene(args.datadir, args.factor, spherify=args.spherify, n_pose_video=llff.n_pose_video_from_flag(args.n_pose_video),
                                decode=png_reader(args))
    except llff.LLFFError as e:
        raise SystemExit(str(e))
    H, W, focal = scene.hwf                                   # main.py:898: of poses[0]
    i_train, i_val, i_test, near, far = llff_split_and_bounds(scene, args.llffhold, args.no_ndc)
    ndc = not args.no_ndc
    batches = RayBatches(scene.bytes[i_train], scene.poses[i_train][:, :3, :4], focal, args.N_rand, ndc, log=log)
    step_args = {}

    def draw(i):
        rays_o, rays_d, viewdirs, target = batches.next()
        step_args['viewdirs'] = viewdirs                      # run_iterations hands step_args to trainer.step beside the batch
        return rays_o, rays_d, target

    loaded = (f'Loaded llff {tuple(scene.bytes.shape)} from "{args.datadir}": {len(i_train)} train / {len(i_val)} val / {len(i_test)} test '
              f'images, {H} x {W}, focal {focal:.4f}; {batches.n} training rays, near {near:.4f} far {far:.4f}{", NDC" if ndc else ""}')
    return dict(hwf=(H, W, focal), bounds=(near, far), ndc=ndc, max_rays=min(args.N_rand, batches.n), draw=draw, step_args=step_args,
                loaded=loaded, test=(torch.from_numpy(scene.poses[i_test][:, :3, :4].copy()), torch.from_numpy(scene.images[i_test])))


def train(args, log=print):
    """main.py without --render_only for --model_name nerf: returns the path of the last checkpoint"""
    from .frontend import load_checkpoint
    start, ckpt = 0, None
    if args.pretrained_ckpt:
        ckpt = load_checkpoint(args.pretrained_ckpt)
        if args.resume:
            start = int(ckpt['global_step'])
    check_supported(args, start)
    data = _llff_data(args, log) if args.dataset_type == 'llff' else _blender_data(args, start, log)
    near, far = data['bounds']
    trainer = trainer_from_args(args, data['max_rays'], near, far)
    best_psnr, best_psnr_step = 0., 0
    if ckpt is not None:
        trainer.load_state_dicts(ckpt['network_fn_state_dict'], ckpt.get('network_fine_state_dict'))
        log(f'Load pretrained ckpt successfully: "{args.pretrained_ckpt}".')
        if args.resume:                                       # main.py:504-509
            trainer.load_optimizer_state_dict(ckpt['optimizer_state_dict'])
            best_psnr, best_psnr_step = float(ckpt.get('best_psnr', 0.)), int(ckpt.get('best_psnr_step', 0))
            log('Resume optimizer successfully.')
    else:
        trainer.load_state_dicts(*trainer.init_state_dicts())
    weights_dir = os.path.join(args.basedir, args.expname or 'train_teacher', 'weights')
    os.makedirs(weights_dir, exist_ok=True)
    log(f'{data["loaded"]}; {args.N_rand} rays per step, {args.N_samples} + {args.N_importance} samples; {trainer.n_param} '
        f'parameters, {trainer.activation_bytes() / 2 ** 30:.2f} GiB of saved activations')

    def test_pass(i):                         # no further [TEST] fields, no line after it
        test_psnr, test_psnr_v2 = eval_test_split(trainer, args, data['hwf'], *data['test'], near=near, far=far, ndc=data['ndc'])
        return test_psnr, test_psnr_v2, '', None

    video_pass = None
    if getattr(args, 'write_video', False):   # main.py:1474-1499, the rgb video; the disparity video is not built
        from . import video as V
        V.check_video_args(args)
        v_poses, v_hwf = V.training_video_poses(args, hwf=data['hwf'])
        expdir = os.path.dirname(weights_dir)

        def video_pass(i):
            eng = test_engine(trainer, args, v_hwf, near, far, data['ndc'])
            return V.video_pass(i, args, expdir, log, v_poses, v_hwf, lambda pose, out: out.copy_(eng.render(pose[:3, :4])['rgb_map'].view(-1, 3)))

    step_args = data['step_args']
    step_args['raw_noise_std'] = args.raw_noise_std
    # the [TRAIN] line's psnr is of img2mse(rgb) alone (main.py:1377-1379)
    return run_iterations(args, trainer, start, (best_psnr, best_psnr_step), weights_dir, log, draw=data['draw'],
                          after_step=lambda batch, loss_rgb: float(loss_rgb.item()), test_pass=test_pass, step_args=step_args,
                          video_pass=video_pass)


def main(argv=None):
    from . import dist as D
    from .frontend import parse_args
    args = parse_args(argv)
    if args.render_only:
        raise SystemExit('train_teacher.py trains; render with main.py --model_name nerf --render_only --pretrained_ckpt X.tar')
    check_supported(args)
    torch.cuda.set_device(D.local_device(0))
    if args.dist_seed >= 0:     # the one process of this trainer: numpy's and torch's generators (host and device) as dist.seed_all seeds every rank's
        np.random.seed(args.dist_seed)
        torch.manual_seed(args.dist_seed)
    train(args, log=lambda *a, **k: print(*a, **k, flush=True))
    return 0

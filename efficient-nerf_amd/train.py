"""Training of the R2L student (main.py:1136-1513 with --model_name R2L / nerf_v3.2 and --data_mode rays): forward pass, backward
pass, rgb loss and Adam as launches of the library's fp32 kernels (csrc/r2l_train.hip, include/r2l_hip.h).

R2LTrainer holds every parameter in one flat device buffer (and likewise the gradients and Adam's two moments) with per-tensor
views, plus the saved output of every layer for the backward pass.  torch supplies the buffers, the stream, the random draws
(t_rand, the batch order) and index selection (the hard-ray pool's sort); every number of a step is computed by the library, in
exact fp32 on the fp32 MFMA, and a step is bit-identical from run to run (the weight gradients are reduced over the rays in slabs
that are added in a fixed order, not with atomics).

The network description is generic.v3_2_plan's: every shape the reference's constructor accepts.
"""
import argparse
import json
import math
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from ._lib import R2LError, check, current_stream, dptr, lib
from .flat_trainer import FlatAdam, init_linears
from .generic import _act_code, _strip, v3_2_plan


def jitter_z_vals(z_vals_dev, n, t_rand=None):
    """PointSampler.sample_train's perturb > 0 branch (model/nerf_raybased.py:117-123): z [n, n_sample] on the device.
    t_rand [n, n_sample] in [0, 1): the caller's, or a torch.rand draw on the device."""
    S = z_vals_dev.shape[0]
    dev = z_vals_dev.device
    if t_rand is None:
        t_rand = torch.rand((n, S), dtype=torch.float32, device=dev)
    t_rand = t_rand.to(dev, torch.float32).contiguous()
    if tuple(t_rand.shape) != (n, S):
        raise R2LError(f't_rand is {tuple(t_rand.shape)}, expected {(n, S)}')
    z = torch.empty((n, S), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().r2l_train_jitter_z(dptr(z_vals_dev), dptr(t_rand), n, S, dptr(z), current_stream()))
    return z


def init_state_dict(plan, seed=None):
    """nn.Linear's default initialisation for every layer of a v3_2_plan, in plan order (what the reference's constructor leaves
    in a freshly built NeRF_v3_2)."""
    return init_linears([(p['key'], p['in_dim'], p['out_dim']) for p in plan], seed)


class R2LTrainer(FlatAdam):
    """NeRF_v3_2 + PointSampler + PositionalEmbedder + MSE loss + torch.optim.Adam(betas (0.9, 0.999)) on the device.

    max_rays: the largest batch a step may carry (the buffers are allocated once, at load_state_dict)."""

    def __init__(self, near=2., far=6., n_sample=16, L=10, netdepth=88, netwidth=256, layerwise_netwidths='', act='relu',
                 use_residual=True, trial=None, max_rays=1 << 14, device=None, z_vals=None):
        self._set_device(device, max_rays)
        self.n_sample, self.L = int(n_sample), int(L)
        if not 1 <= self.L <= 16 or self.n_sample < 1:
            raise R2LError(f'n_sample={n_sample} multires={L}')
        self.input_dim = 3 * self.n_sample * (2 * self.L + 1)
        self.use_residual = bool(use_residual)
        self.plan = v3_2_plan(netdepth, netwidth, self.input_dim, 3, layerwise_netwidths, act, use_residual, trial)
        if len(self.plan) == 2 and self.use_residual:
            raise R2LError('an empty body with --use_residual (netdepth < 4) is not built')
        if z_vals is None:       # model/nerf_raybased.py:88-90, on the host as the reference does
            t_vals = torch.linspace(0., 1., steps=self.n_sample)
            z_vals = float(near) * (1 - t_vals) + float(far) * t_vals
        self.z_vals = torch.as_tensor(z_vals).detach().to('cpu', torch.float32).contiguous()
        # the first layer of the block a block_out layer closes
        self._block_start = {}
        start = None
        for i, p in enumerate(self.plan):
            if p.get('block_in'):
                start = i
            if p.get('block_out'):
                self._block_start[i] = start
        self._set_layout([(p['key'], p['in_dim'], p['out_dim']) for p in self.plan])       # model.parameters() order

    # ---- state -------------------------------------------------------------------------------------------------------------
    @property
    def flops_per_ray(self):
        """of the forward pass; a training step is about three times that (g_x and g_W cost one forward each)"""
        return 2 * sum(p['in_dim'] * p['out_dim'] for p in self.plan)

    def activation_bytes(self, n=None):
        n = self.max_rays if n is None else n
        return 4 * n * (sum(p['out_dim'] for p in self.plan) + self.input_dim + 4 * self.n_sample)

    def _allocate(self):
        n, dev = self.max_rays, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        wmax = max(max(p['out_dim'], p['in_dim']) for p in self.plan[1:])
        slabs = lib().r2l_train_grad_weight_slabs(n)
        ws_floats = max(1, slabs * max(p['out_dim'] * p['in_dim'] + p['out_dim'] for p in self.plan))
        want = self.activation_bytes() + 4 * (4 * self.n_param + 4 * n * wmax + ws_floats + 8 * n)
        try:
            with torch.cuda.device(dev):
                self._allocate_flat()
                self._acts = [torch.empty((n, p['out_dim']), **f32) for p in self.plan]
                self._emb = torch.empty((n, self.input_dim), **f32)
                self._pts = torch.empty((n, 3 * self.n_sample), **f32)
                self._gbuf = [torch.empty((n, wmax), **f32) for _ in range(4)]     # R, Y, Z, P of forward_backward
                self._gtail = torch.empty((n, 3), **f32)
                self._err = torch.empty((n,), **f32)
                self._loss = torch.zeros((1,), **f32)
                self._ws = torch.empty((ws_floats,), **f32)
                self._loss_ws = torch.empty(((n + 255) // 256,), **f32)
                self._z_dev = self.z_vals.to(dev)
        except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
            self._release_flat()
            raise R2LError(f'cannot allocate the training buffers for {n} rays per step: about {want / 2 ** 30:.1f} GiB (saved layer '
                           f'outputs {self.activation_bytes() / 2 ** 30:.1f} GiB: {len(self.plan)} layers; slab workspace '
                           f'{4 * ws_floats / 2 ** 30:.2f} GiB): {e}. Lower --N_rand or the hard-ray share.') from e

    def load_state_dict(self, state_dict):
        sd = _strip(state_dict)
        missing = [k for k in self._slices if k not in sd]
        if missing:
            raise R2LError(f'state_dict lacks {len(missing)} tensors, e.g. {missing[:3]} (has e.g. {sorted(sd)[:4]})')
        for k, (_, _, shape) in self._slices.items():
            if tuple(sd[k].shape) != tuple(shape):
                raise R2LError(f'{k} is {tuple(sd[k].shape)}, the flags describe {tuple(shape)}')
        if self._param is None:
            self._allocate()
        for k, v in self.p.items():
            v.copy_(torch.as_tensor(sd[k]).detach().to(torch.float32))
        return self

    def state_dict(self):
        """The weights on the host, keyed as the reference's network_fn_state_dict."""
        self._need_state()
        return OrderedDict((k, v.detach().cpu().clone()) for k, v in self.p.items())

    def checkpoint_networks(self):
        return pair_networks(self.state_dict())

    # ---- one step ----------------------------------------------------------------------------------------------------------
    def forward(self, emb, n):
        """NeRF_v3_2.forward (model/nerf_raybased.py:539-544) keeping every layer's output; returns rgb [n, 3] (a view)."""
        acts = [a[:n] for a in self._acts]
        plan = self.plan
        self._linear(plan[0]['key'], emb, acts[0], _act_code(plan[0]['act']), None, plan[0].get('res_scale', 1.0))
        cur = acts[0]
        last_body = len(plan) - 2
        for i in range(1, len(plan)):
            p = plan[i]
            body = i <= last_body
            if body and p.get('block_in'):
                cur = acts[i - 1]
            self._linear(p['key'], acts[i - 1], acts[i], _act_code(p['act']), cur if body and p.get('block_out') else None,
                         p.get('res_scale', 1.0), acts[0] if (i == last_body and self.use_residual) else None)
        return acts[-1]

    def embed(self, rays_o, rays_d, perturb=1., t_rand=None):
        """positional_embedder(point_sampler.sample_train(rays_o, rays_d, perturb)) into the trainer's buffer: [n, input_dim]"""
        self._need_state()
        n = rays_o.shape[0]
        ro, rd = self._on_device(n, rays_o=rays_o, rays_d=rays_d)
        pts, emb = self._pts[:n], self._emb[:n]
        with torch.cuda.device(self.device):
            if perturb > 0.:
                z = jitter_z_vals(self._z_dev, n, t_rand)
                check(lib().r2l_sample_points(dptr(ro), dptr(rd), n, dptr(z), self.n_sample, 1, dptr(pts), current_stream()))
            else:
                check(lib().r2l_sample_points(dptr(ro), dptr(rd), n, dptr(self._z_dev), self.n_sample, 0, dptr(pts), current_stream()))
            check(lib().r2l_embed(dptr(pts), n, 3 * self.n_sample, self.L, dptr(emb), current_stream()))
        return emb

    def forward_backward(self, rays_o, rays_d, target, perturb=1., t_rand=None):
        """loss (a one-element device tensor) of the batch; the gradients are left in the flat buffer (grads())."""
        emb = self.embed(rays_o, rays_d, perturb, t_rand)
        return self.forward_backward_embedded(emb, target)

    def forward_backward_embedded(self, emb, target):
        self._need_state()
        n = emb.shape[0]
        tgt, = self._on_device(n, target=target)
        plan, nl = self.plan, len(self.plan)
        last_body = nl - 2
        with torch.cuda.device(self.device):
            rgb = self.forward(emb, n)
            acts = [a[:n] for a in self._acts]
            R, Y, Z, P = (b[:n] for b in self._gbuf)
            # loss, and through the tail's sigmoid: the tail layer's g_z
            gz = self._gtail[:n]
            self._mse_loss(rgb, tgt, 1, gz, self._loss, self._err[:n])
            self._grad_weight(plan[-1]['key'], gz, acts[-2])
            g_y = R[:, :plan[-1]['in_dim']]
            self._grad_input(plan[-1]['key'], gz, g_y, False)
            # body, last layer first.  `stream`: the buffer the gradient of the open block's input is collected in (g_res, then
            # the g_x of the block's first layer on top); P: the same for the head's output under --use_residual (g_post)
            stream = None
            for i in range(last_body, 0, -1):
                p = plan[i]
                w_out, w_in = p['out_dim'], p['in_dim']
                has_res, has_post = bool(p.get('block_out')), i == last_body and self.use_residual
                g_res = res_acc = None
                if has_res:
                    if self.use_residual and self._block_start[i] == 1:
                        g_res, res_acc = P[:, :w_out], True          # block 0's input is the head's output: joins g_post
                    else:
                        g_res, res_acc = g_y, False                  # in place: g_u over g_y
                    stream = g_res
                z = Z[:, :w_out]
                self._act_backward(p['key'], g_y, acts[i], z, _act_code(p['act']), acts[0] if has_post else None,
                                   p.get('res_scale', 1.0) if has_res else 1.0, g_res, res_acc, P[:, :w_out] if has_post else None)
                self._grad_weight(p['key'], z, acts[i - 1])
                if p.get('block_in'):
                    dst, acc = stream, True
                elif i == 1 and self.use_residual:
                    dst, acc = P[:, :w_in], True
                else:
                    dst, acc = Y[:, :w_in], False
                self._grad_input(p['key'], z, dst, acc)
                g_y = dst
            # head: no g_x (the embedding has no parameters)
            z = Z[:, :plan[0]['out_dim']]
            self._act_backward(plan[0]['key'], g_y, acts[0], z, _act_code(plan[0]['act']))
            self._grad_weight(plan[0]['key'], z, emb)
        return self._loss

    def step(self, rays_o, rays_d, target, lr, perturb=1., t_rand=None):
        """forward_backward + Adam.  Returns (loss [1], err [n]): views of the trainer's buffers, valid until the next step;
        err[r] = mean over the channels of (rgb - target)^2 from this step's forward pass (what the hard-ray pool sorts)."""
        loss = self.forward_backward(rays_o, rays_d, target, perturb, t_rand)
        self.adam(lr)
        return loss, self._err[:rays_o.shape[0]]

    @property
    def rgb(self):
        """the last forward pass's output buffer [max_rays, 3]"""
        return self._acts[-1]

    # ---- rendering from the live weights -----------------------------------------------------------------------------------
    def render_rays(self, rays_o, rays_d, out=None):
        """rgb [n, 3] of given rays from the weights as they stand in the flat buffer: PointSampler.sample_train without
        perturbation -> embedding -> the training step's own forward launches, in chunks of at most max_rays.  The weights do not
        leave the device and nothing is drawn.  The chunks run in the step's per-ray buffers (points, embedding, layer outputs),
        all of which the next step's forward pass rewrites before its backward pass reads them; the gradients, Adam's moments,
        the loss and the per-ray error are not touched."""
        self._need_state()
        n = rays_o.shape[0]
        ro, rd = self._on_device(n, limit=False, rays_o=rays_o, rays_d=rays_d)
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            for s in range(0, n, self.max_rays):
                m = min(self.max_rays, n - s)
                out[s:s + m].copy_(self.forward(self.embed(ro[s:s + m], rd[s:s + m], perturb=0.), m))
        return out

    def render(self, c2w, H, W, focal, out=None):
        """rgb [H * W, 3] of one pose (render_func, main.py:401-404) from the live weights"""
        from .teacher import get_rays
        ro, rd = get_rays(int(H), int(W), float(focal), torch.as_tensor(c2w)[:3, :4], device=self.device)
        return self.render_rays(ro.view(-1, 3), rd.view(-1, 3), out=out)


class ShardedStep:
    """A trainer's step on the ranks of one torch.distributed group: the loop is replicated, the rays are sharded.  Every rank hands
    step() the same full batch; it draws t_rand for all n rays (the draw one rank makes), runs forward_backward on its slice
    dist.row_shard(n, rank, world), exchanges (FlatAdam.exchange_gradients: the ranks' gradients added in rank order) and runs Adam: the
    same update of the same bits on every rank.  Returns (loss [1], err [n]) of the whole batch, as R2LTrainer.step does.  Everything
    else (state_dict, render, checkpoint_networks, ...) is the trainer's own."""

    def __init__(self, trainer, group=None):
        import torch.distributed as td
        self.trainer, self.group = trainer, group
        self.rank, self.world = td.get_rank(group), td.get_world_size(group)

    def __getattr__(self, name):
        return getattr(self.__dict__['trainer'], name)

    def step(self, rays_o, rays_d, target, lr, perturb=1., t_rand=None):
        from .dist import row_shard
        tr = self.trainer
        n = rays_o.shape[0]
        r0, r1 = row_shard(n, self.rank, self.world)
        if perturb > 0. and t_rand is None:
            with torch.cuda.device(tr.device):
                t_rand = torch.rand((n, tr.n_sample), dtype=torch.float32, device=tr.device)       # jitter_z_vals' draw for n rays
        if r1 > r0:
            tr.forward_backward(rays_o[r0:r1], rays_d[r0:r1], target[r0:r1], perturb, None if t_rand is None else t_rand[r0:r1])
        loss, err = tr.exchange_gradients(self.group, r1 - r0, n)
        tr.adam(lr)
        return loss, err


def refuse_more_ranks_than_rays(world, n_rays):
    if world > n_rays:
        raise SystemExit(f'{world} ranks for steps of {n_rays} rays: a rank without rays has nothing to do; lower --gpus or raise --N_rand')


# ---------------------------------------------------------------------------------------------------------------------------
# the loop of main.py:1136-1513
# ---------------------------------------------------------------------------------------------------------------------------
def learning_rate(step, lrate, lrate_decay, warmup_lr=''):
    """main.py:1181-1195: linear warm-up from start_lr to lrate until end_iter, then 0.1 ** ((step - end_iter) / (lrate_decay * 1000))"""
    decay_rate = 0.1
    decay_steps = lrate_decay * 1000
    if warmup_lr:
        start_lr, end_iter = [float(x) for x in warmup_lr.split(',')]
        if step < end_iter:
            return (lrate - start_lr) / end_iter * step + start_lr
        return lrate * (decay_rate ** ((step - end_iter) / decay_steps))
    return lrate * (decay_rate ** (step / decay_steps))


def parse_hard_ratio(text):
    """option.py:379-383: '' -> None, 'r' -> float, 'in,out' -> [float, float]"""
    if text in ('', None):
        return None
    if isinstance(text, (float, int, list)):
        return text
    return [float(x) for x in text.split(',')] if ',' in text else float(text)


class HardRayPool:
    """The hard-ray pool of main.py:1325-1347, 1410-1425: rows [rays_o | rays_d | target].  Until it holds batch_size * hard_mul
    rows the n_hard_in worst rays of every batch are appended; from then on every batch is extended by n_hard_out rows drawn from
    the pool, and n_hard_in of those drawn are replaced by the batch's worst rays."""

    def __init__(self, hard_ratio, hard_mul=1.):
        self.hard_ratio, self.hard_mul = parse_hard_ratio(hard_ratio), float(hard_mul)
        self.rows = None
        self.full = False
        self._ix_out = None

    def counts(self, batch_size):
        if isinstance(self.hard_ratio, list):
            n_in, n_out = int(self.hard_ratio[0] * batch_size), int(self.hard_ratio[1] * batch_size)
        else:
            n_in = n_out = int(self.hard_ratio * batch_size)
        return min(n_in, n_out), n_out

    def draw(self, batch_size):
        """rows [n_hard_out, 9] to append to the batch, or None while the pool fills"""
        if not self.full:
            return None
        _, n_out = self.counts(batch_size)
        self._ix_out = np.random.permutation(self.rows.shape[0])[:n_out]
        return self.rows[torch.as_tensor(self._ix_out, device=self.rows.device)]

    def update(self, err, rays_o, rays_d, target, batch_size):
        """err [>= batch_size]: the per-ray error of this step; only the batch's own rays (the first batch_size) are candidates"""
        n_in, _ = self.counts(batch_size)
        if n_in <= 0:
            return
        _, indices = torch.sort(err[:batch_size])
        hard = indices[-n_in:]
        rows = torch.cat([rays_o[hard], rays_d[hard], target[hard]], dim=-1)
        if self.full:
            self.rows[torch.as_tensor(self._ix_out[:n_in], device=self.rows.device)] = rows
        else:
            self.rows = rows if self.rows is None else torch.cat([self.rows, rows], dim=0)
            if self.rows.shape[0] >= batch_size * self.hard_mul:
                self.full = True


def _infinite_order(n):
    """main.py:759-767"""
    order = np.random.permutation(n)
    i = 0
    while True:
        yield order[i]
        i += 1
        if i == n:
            order = np.random.permutation(n)
            i = 0


def pair_networks(coarse, fine=None):
    """the checkpoint's network entries of a coarse / fine pair of state dicts (main.py:1531-1533)"""
    nets = {'network_fn_state_dict': dict(coarse)}
    if fine is not None:
        nets['network_fine_state_dict'] = dict(fine)
    return nets


def save_train_checkpoint(path, trainer, global_step, best_psnr=0, best_psnr_step=0):
    """The reference's schema (main.py:1516-1542) with the optimizer's state; without the pickled module, which the reference
    only reads when it is there (main.py:484)."""
    # a trainer names the networks of its checkpoint; an object that only offers the teacher's state_dicts() pair is read as that
    nets = trainer.checkpoint_networks() if hasattr(trainer, 'checkpoint_networks') else pair_networks(*trainer.state_dicts())
    to_save = {'global_step': int(global_step), 'best_psnr': best_psnr, 'best_psnr_step': best_psnr_step,
               'network_fn_state_dict': nets['network_fn_state_dict'], 'optimizer_state_dict': trainer.optimizer_state_dict()}
    to_save.update(nets)          # the teacher's network_fine_state_dict goes behind them (main.py:1531-1533)
    tmp = path + '.tmp'
    torch.save(to_save, tmp)
    os.replace(tmp, path)
    return path


def refuse_negative_i_testset(args):
    if args.i_testset < 0:
        raise SystemExit(f'--i_testset {args.i_testset}: a positive interval, or 0 for no test renders')


def run_iterations(args, trainer, start, best, weights_dir, log, *, draw, after_step, test_pass=None,
                   ckpt_name=lambda it: 'ckpt.tar', step_args={}, writer=True, guard=None, video_pass=None):
    """Iterations start + 1 .. N_iters of main.py:1136-1513 on either trainer: the learning rate, the step, the [TRAIN] line, the
    test renders every --i_testset iterations (0: none) with the best checkpoint and the [TEST] line, the periodic and the final
    checkpoint.  Returns the path of the last checkpoint written.  What differs between the trainers comes in as
      draw(i)                   -> (rays_o, rays_d, target) of iteration i on the device; its time is the line's data_time
      after_step(batch, second) -> the mse the line's psnr is of, or None for the loss; second: what trainer.step returned second
      test_pass(i)              -> (test_psnr, test_psnr_v2, further fields of the [TEST] line, a line to log after it or None)
      ckpt_name(i)              -> the periodic checkpoint's file name
      video_pass(i)             -> renders and writes the video of iteration i (every --i_video iterations, 0: never; --write_video)
    best: (best_psnr, best_psnr_step) so far; step_args: passed on to trainer.step beside perturb.
    On the ranks of a ray-sharded run every rank runs this loop on the same batches: writer is True on the one rank that renders the
    test split and writes files (the others go on to the next step's collective), and guard(i) is entered by every rank before
    anything is written at iteration i (it raises on every rank when their weights differ); test_pass, and likewise video_pass, is
    then given on every rank or on none."""
    from .frontend import mse2psnr
    best_psnr, best_psnr_step = best
    save = lambda name, it: save_train_checkpoint(os.path.join(weights_dir, name), trainer, it, best_psnr, best_psnr_step)
    guarded = [None]

    def agree(it):
        if guard is not None and guarded[0] != it:
            guard(it)
            guarded[0] = it
    hist_psnr = 0.
    path = None
    log('Begin training')
    for i in range(start + 1, args.N_iters + 1):
        t0 = time.time()
        lr = learning_rate(i, args.lrate, args.lrate_decay, args.warmup_lr)
        batch = draw(i)
        t_data = time.time() - t0
        loss, second = trainer.step(*batch, lr, perturb=args.perturb, **step_args)
        mse = after_step(batch, second)
        loss_v = float(loss.item())
        t_batch = time.time() - t0
        if not math.isfinite(loss_v):
            raise R2LError(f'the loss is {loss_v} at iteration {i} (LR {lr:.10f})')
        psnr = mse2psnr(loss_v if mse is None else mse)
        hist_psnr = psnr if i == start + 1 else hist_psnr * 0.95 + psnr * 0.05
        if i % args.i_print == 0:
            log(f'[TRAIN] Iter {i} data_time {t_data:.4f} batch_time {t_batch:.4f} loss {loss_v:.6f} psnr {psnr:.4f} hist_psnr {hist_psnr:.4f} '
                f'LR {lr:.10f}')
        testing = test_pass is not None and args.i_testset and i % args.i_testset == 0
        if testing:
            agree(i)
        if testing and writer:                                                          # main.py:1442-1471
            log(f'Iter {i} Testing...')
            t_ = time.time()
            test_psnr, test_psnr_v2, fields, after = test_pass(i)
            t_test = time.time() - t_
            if test_psnr_v2 > best_psnr:                      # main.py:1458
                best_psnr, best_psnr_step = test_psnr_v2, i
                best_path = save('ckpt_best.tar', i)
                log(f'Iter {i} Save the best checkpoint: "{best_path}".')
            log(f'[TEST] Iter {i} TestPSNR {test_psnr:.4f} TestPSNRv2 {test_psnr_v2:.4f} BestPSNRv2 {best_psnr:.4f} (Iter {best_psnr_step}) '
                f'{fields}TrainHistPSNR {hist_psnr:.4f} LR {lr:.8f} Time {t_test:.1f}s')
            if after:
                log(after)
        videoing = video_pass is not None and args.i_video and i % args.i_video == 0      # main.py:1474-1499
        if videoing:
            agree(i)
        if videoing and writer:
            video_pass(i)
        if i % args.i_weights == 0:
            agree(i)
            if writer:
                path = save(ckpt_name(i), i)
                log(f'Iter {i} Save checkpoint: "{path}".')
    if args.N_iters > start:
        agree(args.N_iters)
        if writer and args.N_iters % args.i_weights != 0:
            path = save(ckpt_name(args.N_iters), args.N_iters)
            log(f'Iter {args.N_iters} Save checkpoint: "{path}".')
    return path


def trainer_from_args(args, max_rays):
    if args.dataset_type == 'blender':
        near, far = 2., 6.          # main.py:930-931
    elif args.dataset_type == 'llff' and not args.no_ndc:
        near, far = 0., 1.          # main.py:917-919: the student samples world-space rays of the loader's frame at depths in [0, 1]
    elif args.trial.near > 0 and args.trial.far > 0:
        near, far = args.trial.near, args.trial.far
    else:
        raise R2LError(f'dataset_type={args.dataset_type}: training takes near / far from --trial.near and --trial.far')
    if args.trial.near > 0:
        near = args.trial.near
    if args.trial.far > 0:
        far = args.trial.far
    if args.plucker or args.learn_depth or args.linear_tail:
        raise R2LError('plucker / learn_depth / linear_tail variants are not built')
    trial = None
    if args.trial.ON:
        trial = dict(body_arch=args.trial.body_arch, n_block=args.trial.n_block, n_learnable=int(args.trial.n_learnable),
                     res_scale=float(args.trial.res_scale), inact=args.trial.inact, outact=args.trial.outact)
    return R2LTrainer(near, far, n_sample=args.n_sample_per_ray, L=args.multires, netdepth=args.netdepth, netwidth=args.netwidth,
                      layerwise_netwidths=args.layerwise_netwidths, act=args.act, use_residual=args.use_residual, trial=trial,
                      max_rays=max_rays)


def load_test_split(args, device=None):
    """The test split the loop renders every --i_testset iterations (main.py:922-937, 1004-1012): ((poses, (H, W, focal), gt
    [N, H, W, 3] on `device`), None), or (None, what is missing) when there is no test split to load.  A transforms_test.json
    whose images are not there is an error: a half-copied scene must not train without the validation it asked for."""
    from . import blender
    if args.dataset_type == 'llff':      # main.py:891-911, 1005: the held-out views of the scene under --datadir
        from .frontend import has_llff_scene, load_llff_set
        if not has_llff_scene(args):
            return None, (f'"{os.path.join(args.datadir, "poses_bounds.npy")}" (--dataset_type llff' +
                          (', and --synthetic_poses is set' if args.synthetic_poses > 0 else '') + ')')
        view = argparse.Namespace(**vars(args))
        view.render_test = True
        poses, hwf, gt = load_llff_set(view)
        return (poses, hwf, gt if device is None else gt.to(device)), None
    if args.dataset_type != 'blender':
        return None, f'--dataset_type {args.dataset_type} (test renders are built for --dataset_type blender and llff)'
    tf = os.path.join(args.datadir, 'transforms_test.json')
    if not os.path.exists(tf):
        return None, f'"{tf}"'
    with open(tf) as fp:
        frames = json.load(fp)['frames']
    from .frontend import png_reader
    lost = [p for p in (os.path.join(args.datadir, f['file_path'] + '.png') for f in frames[::args.testskip or 1]) if not os.path.exists(p)]
    if lost:
        raise R2LError(f'"{tf}" names {len(lost)} image(s) that are not there, e.g. "{lost[0]}": complete the scene, or point --datadir elsewhere '
                       f'to train without test renders')
    imgs, poses, hwf, _ = blender.load_blender_data(args.datadir, args.half_res, args.testskip, splits=('test',), decode=png_reader(args))
    gt = blender.composite(imgs, args.white_bkgd)
    return (poses, (int(hwf[0]), int(hwf[1]), float(hwf[2])), gt if device is None else gt.to(device)), None


def eval_test_split(trainer, test, savedir=None, test_flip=False, lpips=None, png_device=False):
    """render_path over the test split from the live weights (main.py:1442-1456): the frames [N, H, W, 3] on the device and
    frontend.test_metrics' test_psnr, test_psnr_v2 and test_ssim; with savedir the frames as <k>.png, with png_device finished on the
    device from the stack where it lies (png.write_pngs).  test: load_test_split's, its ground truth on the trainer's device."""
    from .frontend import frame_errors, stack_flip, stack_lpips, test_metrics, to8b, write_png
    poses, (H, W, focal), gt = test
    rgbs = torch.empty((len(poses), H, W, 3), dtype=torch.float32, device=trainer.device)
    if gt.device != rgbs.device:
        raise R2LError(f'the ground truth is on {gt.device}, the trainer on {rgbs.device}: load_test_split(args, device=trainer.device)')
    mse_dev, ssim_dev = [], []
    for k, pose in enumerate(poses):
        trainer.render(pose, H, W, focal, out=rgbs[k].view(-1, 3))
        mse, ssim = frame_errors(rgbs[k], gt[k])
        mse_dev.append(mse)
        ssim_dev.append(ssim)
    misc = test_metrics(rgbs, gt, mse_dev, ssim_dev)
    if lpips is not None:       # a metrics.LPIPS: reads the frames, writes buffers of its own
        misc['test_lpips'] = stack_lpips(lpips, rgbs, gt)
    if test_flip:               # reads the frames, writes buffers of its own
        misc['test_flip'] = stack_flip(rgbs, gt)
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)
        if png_device:
            from .png import write_pngs
            write_pngs([os.path.join(savedir, f'{k:03d}.png') for k in range(len(rgbs))], rgbs)
            return rgbs, misc
        host = rgbs.cpu().numpy()
        for k in range(len(host)):
            write_png(os.path.join(savedir, f'{k:03d}.png'), to8b(host[k]))
    return rgbs, misc


def train(args, log=print):
    """_train, and whatever ends it, the teacher engine of --kd_online is closed"""
    engines = []
    try:
        return _train(args, log, engines)
    finally:
        for eng in engines:
            if hasattr(eng, 'close'):
                eng.close()


def _train(args, log, engines):
    """main.py without --render_only for --model_name R2L / nerf_v3.2, --data_mode rays; with --kd_online the rays of every step are
    rendered by the teacher on the device (online.py) instead of read from shards, and everything behind them is the same code."""
    from .create_data import BlenderDataset_v2
    from .dist import rank_world, row_shard
    from .frontend import load_checkpoint
    from .metrics import LPIPS, lpips_weights_from_args
    # --test_lpips: refused, or its weights loaded once, before a device is touched (main() has done it already)
    lpips_tensors = args.lpips_tensors if hasattr(args, 'lpips_tensors') else lpips_weights_from_args(args)
    rank, world = rank_world()       # several ranks: the loop is replicated, the rays of a step are sharded (ShardedStep)
    if rank != 0:
        log = lambda *a, **k: None
    online = bool(getattr(args, 'kd_online', False))
    if online:                 # every step's rays from the teacher (online.py) instead of shards
        from .online import check_online_args, source_from_args
        check_online_args(args)
        dataset, split = None, int(args.kd_online_split)
    else:
        if args.data_mode != 'rays':
            raise R2LError(f'--data_mode {args.data_mode}: training is built for --data_mode rays (the shards create_data.py writes)')
        if not args.datadir_kd:
            raise R2LError('training needs --datadir_kd (a directory of ray shards)')
        datadir_kd = args.datadir_kd.split(':')[1] if ':' in args.datadir_kd else args.datadir_kd        # main.py:1052-1053
        dataset = BlenderDataset_v2(datadir_kd, dim_dir=3, dim_rgb=3, pseudo_ratio=args.pseudo_ratio)
        if len(dataset) == 0:
            raise R2LError(f'no .npy shards under {datadir_kd}')
        split = int(dataset[0][0].shape[0])
    batch_size = args.N_rand * split
    pool = HardRayPool(args.hard_ratio, args.hard_mul) if parse_hard_ratio(args.hard_ratio) else None
    n_hard_out = pool.counts(batch_size)[1] if pool else 0
    refuse_negative_i_testset(args)
    refuse_more_ranks_than_rays(world, batch_size)
    max_rays = -(-(batch_size + n_hard_out) // world)         # a rank's slice of the step's rays and of the pool's share
    trainer = trainer_from_args(args, max_rays)
    dev = trainer.device
    if online:
        source, source_desc = source_from_args(args, log=log)
        engines.append(source.engine)
        if world > 1:
            from .online import agree_teacher_precision
            agree_teacher_precision(source.engine)
    if rank == 0:
        test, missing = load_test_split(args, device=dev)        # the ground truth goes to the device once
    else:
        test, missing = None, 'rank 0 renders the test split'
    has_test = test is not None
    flip_on = bool(getattr(args, 'test_flip', False))          # TestFLIP behind TestSSIM (main.py:1468)
    lpips = None                                               # TestLPIPS between them: the context is created once, on the rank that renders
    if lpips_tensors is not None and test is not None:
        with torch.cuda.device(dev):
            lpips = LPIPS(lpips_tensors)
    if world > 1:                # the other ranks enter the agreement guard where rank 0 renders
        import torch.distributed as td
        flag = [has_test]
        td.broadcast_object_list(flag, src=0)
        has_test = flag[0]
    if rank == 0 and args.test_pretrained and (test is None or not args.pretrained_ckpt):
        raise SystemExit('--test_pretrained needs --pretrained_ckpt and a test split: ' +
                         (f'{missing} is not there' if test is None else 'no --pretrained_ckpt was given'))
    start = 0
    best_psnr, best_psnr_step = 0, 0
    if args.pretrained_ckpt:
        ckpt = load_checkpoint(args.pretrained_ckpt)
        trainer.load_state_dict(ckpt['network_fn_state_dict'])
        log(f'Load pretrained ckpt successfully: "{args.pretrained_ckpt}".')
        if args.resume:                                       # main.py:504-509
            start = int(ckpt['global_step'])
            trainer.load_optimizer_state_dict(ckpt['optimizer_state_dict'])
            best_psnr, best_psnr_step = ckpt.get('best_psnr', 0), ckpt.get('best_psnr_step', 0)
            log('Resume optimizer successfully.')
    else:
        trainer.load_state_dict(init_state_dict(trainer.plan))
    expdir = os.path.join(args.basedir, args.expname or 'train')
    weights_dir = os.path.join(expdir, 'weights')
    os.makedirs(weights_dir, exist_ok=True)
    log((f'Online distillation: {source_desc}; {batch_size} rays per step + {n_hard_out} hard rays; ' if online else
         f'Found {len(dataset)} shard(s) of {split} rays under "{datadir_kd}"; {args.N_rand} per step + {n_hard_out} hard rays; ') +
        f'{trainer.n_param} parameters in {len(trainer.plan)} layers, {trainer.activation_bytes() / 2 ** 30:.2f} GiB of saved activations' +
        (f'; {world} ranks, ≤ {max_rays} rays each' if world > 1 else ''))
    if test is None:
        log(f'No test renders during this run: {missing} is not there.')
    else:
        log(f'Test split: {len(test[0])} view(s) {test[1][0]} x {test[1][1]} from "{args.datadir}", ' +
            (f'rendered every {args.i_testset} iterations' if args.i_testset else 'not rendered while training (--i_testset 0)'))
    if args.test_pretrained and rank == 0:                    # main.py:1035-1047
        log('Testing pretrained...')
        _, misc = eval_test_split(trainer, test, test_flip=flip_on, lpips=lpips)
        log(f"Pretrained test: TestPSNR {misc['test_psnr']:.4f} TestPSNRv2 {misc['test_psnr_v2']:.4f}" +
            (f" TestLPIPS {misc['test_lpips']:.4f}" if lpips is not None else '') + (f" TestFLIP {misc['test_flip']:.4f}" if flip_on else ''))
    order = None if online else _infinite_order(len(dataset))

    def draw(i):
        if online:
            rays_o, rays_d, target = source.batch(i, batch_size, rows=row_shard(batch_size, rank, world) if world > 1 else None)
        else:
            items = [dataset[int(next(order))] for _ in range(args.N_rand)]
            rays_o, rays_d, target = (torch.cat([it[k] for it in items], 0).to(dev) for k in range(3))
        if pool is not None:
            picked = pool.draw(batch_size)
            if picked is not None:
                rays_o, rays_d, target = (torch.cat([a, picked[:, 3 * k:3 * k + 3]], 0) for k, a in enumerate((rays_o, rays_d, target)))
        if online:
            torch.cuda.synchronize(dev)       # data_time contains the teacher's render
        return rays_o, rays_d, target

    def after_step(batch, err):               # the psnr is the loss's own
        if pool is not None:
            pool.update(err, *batch, batch_size)

    def test_pass(i):                         # main.py:1442-1456
        testsavedir = os.path.join(expdir, f'testset_iter{i}')
        _, misc = eval_test_split(trainer, test, savedir=testsavedir, test_flip=flip_on, lpips=lpips, png_device=getattr(args, 'png_device', False))
        flip_field = (f"TestLPIPS {misc['test_lpips']:.4f} " if lpips is not None else '') + (f"TestFLIP {misc['test_flip']:.4f} " if flip_on else '')
        return misc['test_psnr'], misc['test_psnr_v2'], f"TestSSIM {misc['test_ssim']:.4f} " + flip_field, f'Saved rendered test images: "{testsavedir}"'

    video_pass = None
    if getattr(args, 'write_video', False):   # on every rank: the others enter the agreement guard where rank 0 renders
        from . import video as V
        V.check_video_args(args)
        if rank == 0:
            v_poses, v_hwf = V.training_video_poses(args, hwf=test[1] if test is not None else None)
            video_pass = lambda i: V.video_pass(i, args, expdir, log, v_poses, v_hwf,
                                                lambda pose, out: trainer.render(pose, *v_hwf, out=out))
        else:
            video_pass = lambda i: None

    stepper, guard = trainer, None
    if world > 1:
        stepper = ShardedStep(trainer)
        guard = lambda it: trainer.check_agreement(None, f' by iteration {it}')
    return run_iterations(args, stepper, start, (best_psnr, best_psnr_step), weights_dir, log, draw=draw, after_step=after_step,
                          test_pass=test_pass if has_test else None,
                          ckpt_name=lambda it: f'ckpt_{it}.tar' if args.save_intermediate_models else 'ckpt.tar',      # main.py:1510
                          writer=rank == 0, guard=guard, video_pass=video_pass)

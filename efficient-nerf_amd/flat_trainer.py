"""What the two trainers (train.R2LTrainer, train_teacher.NeRFTrainer) stand on: the flat parameter layout and its buffers, the
launches of the library's per-layer training entries (forward, g_W, g_x, activation backward, rgb loss, Adam), the checks of a
batch of rays, nn.Linear's initialisation and the optimizer state in torch.optim.Adam's format.  A trainer adds its own saved
activations and its own walk over the layers; no other module calls those entries."""
from collections import OrderedDict

import numpy as np
import torch

from ._lib import R2LError, check, current_stream, dptr, lib
from .generic import _view

ADAM_BETAS = (0.9, 0.999)
ADAM_EPS = 1e-8
ACT_NONE, ACT_RELU = 0, 1         # generic.ACT_CODES


def init_linears(layers, seed=None):
    """nn.Linear's default initialisation of every (name, in_dim, out_dim) of `layers`, in that order (what the reference's
    constructors leave in a freshly built network): name.weight, name.bias.  With a seed, torch's generator is left as found."""
    g = torch.random.get_rng_state()
    if seed is not None:
        torch.manual_seed(seed)
    sd = OrderedDict()
    for name, i, o in layers:
        lin = torch.nn.Linear(i, o)
        sd[name + '.weight'], sd[name + '.bias'] = lin.weight.detach().clone(), lin.bias.detach().clone()
    if seed is not None:
        torch.random.set_rng_state(g)
    return sd


class FlatAdam:
    """Every parameter in one flat device buffer (_param; _grad, _m, _v likewise) cut into per-tensor views by _slices (name ->
    (offset, count, shape), in the reference's model.parameters() order), the per-layer launches keyed by a layer's name (the prefix
    of its two parameter names), one r2l_train_adam launch over the whole buffer, and the state in torch.optim.Adam's format.  A
    trainer allocates what the launches write beside the flat buffers: _ws (the slab workspace of g_W), _loss_ws (the loss's
    partial sums).

    _frozen: names that never receive a gradient (a module the reference builds and its forward never calls).  torch's Adam skips a
    parameter whose .grad is None: it keeps no state for it and never moves it.  Here their gradient stays zero, which the launch
    maps to an update of exactly zero with zero moments; the saved state has no entry for them and a loaded state need not."""
    _frozen = frozenset()
    _min_rays = 0             # the student's launches take an empty batch

    # ---- layout and buffers ------------------------------------------------------------------------------------------------
    def _set_device(self, device, max_rays):
        if not torch.cuda.is_available():
            raise R2LError('no HIP device visible to torch: training has no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_rays = int(max_rays)
        if self.max_rays < 1:
            raise R2LError(f'max_rays={max_rays}')

    def _set_layout(self, layers):
        """layers: (name, in_dim, out_dim) in model.parameters() order; weight then bias, layer by layer"""
        self._dims = OrderedDict((name, (i, o)) for name, i, o in layers)
        self._slices = OrderedDict()
        off = 0
        for name, (i, o) in self._dims.items():
            for kind, shape in (('weight', (o, i)), ('bias', (o,))):
                cnt = int(np.prod(shape))
                self._slices[f'{name}.{kind}'] = (off, cnt, shape)
                off += cnt
        self.n_param = off
        self.t = 0                # Adam updates so far
        self.lr = 0.
        self._param = None

    def state_names(self):
        return list(self._slices)

    def _views(self, flat):
        return OrderedDict((k, flat[o:o + c].view(shape)) for k, (o, c, shape) in self._slices.items())

    def _allocate_flat(self):
        """the four flat buffers and their views; the caller handles a failure (each trainer names its own sizes), after
        _release_flat()"""
        f32 = dict(dtype=torch.float32, device=self.device)
        self._param, self._grad, self._m, self._v = (torch.zeros(self.n_param, **f32) for _ in range(4))
        self.p, self.g = self._views(self._param), self._views(self._grad)
        self.exp_avg, self.exp_avg_sq = self._views(self._m), self._views(self._v)

    def _release_flat(self):
        self._param = self._grad = self._m = self._v = self.p = self.g = self.exp_avg = self.exp_avg_sq = None

    def _need_state(self):
        if self._param is None:
            raise R2LError('the trainer has no weights yet: load_state_dict first')

    def grads(self):
        self._need_state()
        return OrderedDict((k, v.detach().clone()) for k, v in self.g.items())

    def _on_device(self, n, limit=True, **named):
        """the named [n, 3] tensors (rays_o, rays_d, target) of a batch as contiguous float32 on the device"""
        if limit and not self._min_rays <= n <= self.max_rays:
            raise R2LError(f'{n} rays in a step, the buffers were allocated for max_rays = {self.max_rays}')
        out = [t.to(self.device, torch.float32).contiguous() for t in named.values()]
        if any(tuple(t.shape) != (n, 3) for t in out):
            raise R2LError(f"{' / '.join(named)} {'is' if len(out) == 1 else 'are'} {' / '.join(str(tuple(t.shape)) for t in out)}, "
                           f'expected {(n, 3)}')
        return out

    # ---- launches ----------------------------------------------------------------------------------------------------------
    def _linear(self, name, x, y, act, res=None, res_scale=1., post=None):
        """y = act(res_scale * (x W^T + b) + res) + post"""
        i, o = self._dims[name]
        xp, ldx = _view(x, i)
        yp, ldy = _view(y, o)
        rp, ldr = _view(res)
        pp, ldp = _view(post)
        check(lib().r2l_linear_forward_dev(dptr(self.p[name + '.weight']), dptr(self.p[name + '.bias']), o, i, xp, ldx, x.shape[0], yp, ldy,
                                           rp, ldr, float(res_scale), act, pp, ldp, current_stream()))

    def _grad_weight(self, name, gz, x):
        i, o = self._dims[name]
        zp, ldz = _view(gz, o)
        xp, ldx = _view(x, i)
        check(lib().r2l_train_grad_weight(zp, ldz, xp, ldx, x.shape[0], o, i, dptr(self.g[name + '.weight']), dptr(self.g[name + '.bias']),
                                          dptr(self._ws), self._ws.numel(), current_stream()))

    def _grad_input(self, name, gz, gx, accumulate):
        i, o = self._dims[name]
        zp, ldz = _view(gz, o)
        xp, ldx = _view(gx, i)
        check(lib().r2l_train_grad_input(zp, ldz, gz.shape[0], dptr(self.p[name + '.weight']), o, i, xp, ldx, 1 if accumulate else 0,
                                         current_stream()))

    def _act_backward(self, name, g_y, y, g_z, act=ACT_RELU, post=None, scale=1., g_res=None, res_acc=False, g_post=None):
        """g_u = g_y * act'(y - post) from the layer's saved output; g_z = scale * g_u, g_res = g_u (+ g_res), g_post = g_y"""
        w = self._dims[name][1]
        gp, ldg = _view(g_y, w)
        yp, ldy = _view(y, w)
        pp, ldp = _view(post)
        zp, ldz = _view(g_z, w)
        rp, ldr = _view(g_res)
        qp, ldq = _view(g_post)
        check(lib().r2l_train_act_backward(gp, ldg, yp, ldy, pp, ldp, y.shape[0], w, act, float(scale), zp, ldz, rp, ldr,
                                           1 if res_acc else 0, qp, ldq, 0, current_stream()))

    def _mse_loss(self, rgb, target, through_sigmoid, g_rgb, loss, err=None):
        """loss [1] = img2mse(rgb, target) and its gradient at rgb (through the sigmoid that made rgb, or not); err [n] or None"""
        check(lib().r2l_train_mse_loss(dptr(rgb), dptr(target), rgb.shape[0], through_sigmoid, dptr(g_rgb), dptr(err), dptr(loss),
                                       dptr(self._loss_ws), self._loss_ws.numel(), current_stream()))

    def adam(self, lr):
        """One torch.optim.Adam update of every parameter from the gradients in the buffer."""
        self._need_state()
        self.t += 1
        self.lr = float(lr)
        with torch.cuda.device(self.device):
            check(lib().r2l_train_adam(dptr(self._param), dptr(self._grad), dptr(self._m), dptr(self._v), self.n_param, float(lr), self.t,
                                       current_stream()))

    # ---- a step whose rays are sharded over the ranks ------------------------------------------------------------------------
    def exchange_gradients(self, group, n_local, n_total, loss=None, err=None):
        """After forward_backward on this rank's slice dist.row_shard(n_total, rank, world) of a step's rays (n_local of them; an
        empty slice runs no layer launch): ONE all-gather of every rank's [gradient | loss | per-ray error] row into a kept
        [world, row] buffer, then r2l_train_sum_parts over the gradient columns into the flat gradient buffer, parts in rank order
        with the weights n_r / n_total (every rank's loss kernel divided by its own 3 n_r) -- a fixed-order sum, not an all-reduce:
        the same bits on every rank, under either backend, from run to run, and what one process computes that holds all the
        parts.  adam() then runs as on one rank.  An empty slice contributes exact zeros, whatever its buffers held.
        loss [1] / err [>= n_local]: this rank's (default: the trainer's own buffers).
        Returns (the step's loss [1] = sum of w_r loss_r in rank order, written to `loss`; the per-ray error [n_total] in ray order)."""
        import ctypes as C
        import torch.distributed as td
        from . import dist as D
        self._need_state()
        world, rank = td.get_world_size(group), td.get_rank(group)
        loss = self._loss if loss is None else loss
        err = self._err if err is None else err
        bounds, weights = D.shard_weights(n_total, world)
        counts = [b - a for a, b in bounds]
        if n_total < 1 or n_local != counts[rank] or max(counts) > self.max_rays:
            raise R2LError(f'rank {rank} of {world} holds {n_local} of a step\'s {n_total} rays, its slice is {counts[rank]} (max_rays = {self.max_rays})')
        P = self.n_param
        row = (P + 1 + self.max_rays + 3) // 4 * 4          # rows stay 16-byte aligned in the gathered buffer
        if getattr(self, '_xall', None) is None or tuple(self._xall.shape) != (world, row):
            self._xsend = torch.zeros((row,), dtype=torch.float32, device=self.device)
            self._xall = torch.empty((world, row), dtype=torch.float32, device=self.device)
        send = self._xsend
        with torch.cuda.device(self.device):
            if n_local == 0:
                send.zero_()
            else:
                send[:P].copy_(self._grad)
                send[P:P + 1].copy_(loss)
                send[P + 1:P + 1 + n_local].copy_(err[:n_local])
            D.all_gather_into(self._xall, send, group)
            w = (C.c_float * world)(*weights)
            flat = self._xall.view(-1)
            check(lib().r2l_train_sum_parts(dptr(flat), row, world, w, P, dptr(self._grad), current_stream()))
            check(lib().r2l_train_sum_parts(dptr(flat[P:]), row, world, w, 1, dptr(loss), current_stream()))
            err_all = torch.cat([self._xall[r, P + 1:P + 1 + c] for r, c in enumerate(counts)])
        return loss, err_all

    def check_agreement(self, group, what=''):
        """The ranks of a ray-sharded run must hold the same parameters bit for bit: two 64-bit checksums of the parameter buffer's
        words (their sum, and their sum weighted by position) are all-gathered and compared for equality.  Every rank raises when
        any two differ."""
        import torch.distributed as td
        from . import dist as D
        self._need_state()
        bits = torch.cat([self._param, self._m, self._v]).view(torch.int32).to(torch.int64)
        pos = torch.arange(1, bits.numel() + 1, dtype=torch.int64, device=bits.device)
        mine = torch.stack([bits.sum(), (bits * pos).sum()])
        got = D.all_gather_cat(mine[None], group).cpu()
        if not bool((got == got[0]).all()):
            bad = [r for r in range(got.shape[0]) if not bool((got[r] == got[0]).all())]
            raise R2LError(f'the ranks\' weights have diverged{what}: rank(s) {bad} of {td.get_world_size(group)} hold other parameters or Adam '
                           f'moments than rank 0 (checksums {[tuple(int(v) for v in g) for g in got]}); nothing is written from them')

    # ---- the optimizer's state ---------------------------------------------------------------------------------------------
    def optimizer_state_dict(self):
        """torch.optim.Adam.state_dict(): parameters indexed in model.parameters() order (weight then bias, layer by layer)."""
        self._need_state()
        idx = list(range(len(self._slices)))
        state = {}
        if self.t > 0:
            for i, k in enumerate(self._slices):
                if k in self._frozen:
                    continue
                state[i] = {'step': torch.tensor(float(self.t)), 'exp_avg': self.exp_avg[k].detach().cpu().clone(),
                            'exp_avg_sq': self.exp_avg_sq[k].detach().cpu().clone()}
        group = {'lr': float(self.lr), 'betas': ADAM_BETAS, 'eps': ADAM_EPS, 'weight_decay': 0, 'amsgrad': False, 'maximize': False,
                 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None, 'decoupled_weight_decay': False,
                 'params': idx}
        return {'state': state, 'param_groups': [group]}

    def load_optimizer_state_dict(self, osd):
        self._need_state()
        groups = osd.get('param_groups', [])
        n_par = sum(len(g['params']) for g in groups)
        if n_par != len(self._slices):
            raise R2LError(f'the optimizer state describes {n_par} parameters, this network has {len(self._slices)}')
        for g in groups:
            if tuple(g.get('betas', ADAM_BETAS)) != ADAM_BETAS or g.get('eps', ADAM_EPS) != ADAM_EPS or g.get('weight_decay', 0) != 0 \
                    or g.get('amsgrad', False):
                raise R2LError(f"the Adam built here has betas {ADAM_BETAS}, eps {ADAM_EPS}, no weight decay, no amsgrad; the state has "
                               f"betas {g.get('betas')} eps {g.get('eps')} weight_decay {g.get('weight_decay')} amsgrad {g.get('amsgrad')}")
        order = [i for g in groups for i in g['params']]
        state = osd.get('state', {})
        self._m.zero_()
        self._v.zero_()
        steps = set()
        for pos, k in zip(order, self._slices):
            st = state.get(pos)
            if st is None:
                continue
            for name, dst in (('exp_avg', self.exp_avg[k]), ('exp_avg_sq', self.exp_avg_sq[k])):
                if tuple(st[name].shape) != tuple(dst.shape):
                    raise R2LError(f'optimizer state {pos} ({k}) {name} is {tuple(st[name].shape)}, expected {tuple(dst.shape)}')
                dst.copy_(st[name].detach().to(torch.float32))
            steps.add(int(float(st['step'])))
        n_live = len(self._slices) - len(self._frozen)
        if len(steps) > 1 or (steps and not n_live <= len(state) <= len(self._slices)):
            raise R2LError(f'the optimizer state carries step counts {sorted(steps)} over {len(state)} of {n_live} trained parameters: '
                           f'one flat Adam launch needs one count for all of them')
        self.t = steps.pop() if steps else 0
        if groups:
            self.lr = float(groups[0].get('lr', self.lr))
        return self

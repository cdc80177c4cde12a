"""Host-side mirror of the reference's R2L call surface, backed by libr2l_hip.so.

Reference interface mirrored (MingSun-Tse/Efficient-NeRF):
  PointSampler            model/nerf_raybased.py:76-126
  PositionalEmbedder      model/nerf_raybased.py:191-208
  NeRF_v3_2               model/nerf_raybased.py:480-544
  render_func             main.py:401-404
  render_path R2L branch  main.py:285-325

The reference evaluates ``model(positional_embedder(point_sampler.sample_test(c2w)))`` as
three eager stages that materialise [N,48] and [N,1008] tensors.  Here the three calls
compose lazily: ``sample_test`` returns a ``LazyPoints`` handle, the embedder wraps it,
and the model launches ONE fused HIP kernel (get_rays + sampling + embedding + ResMLP)
that writes [N,3].  Calling ``.materialize()`` (or torch ops via ``.tensor``) on the lazy
handles runs the stand-alone HIP kernels instead, which is what the parity tests do.
"""
import ctypes as C
import math
import sys

import torch

from . import _lib
from ._lib import (R2LError, PREC_FP16X1, PREC_FP16X3, PREC_FP16_FP8, PREC_FP16_E4M3, PREC_FP16X3_ASM, PREC_FP16_SPLIT, PREC_FP16_SPLIT8, check, current_stream,
                   dptr, lib)

SPLIT_MODES = (PREC_FP16_FP8, PREC_FP16_E4M3, PREC_FP16_SPLIT, PREC_FP16_SPLIT8)   # generated head launch + generated body kernel, calibrated operand scales
TWO_PART = (PREC_FP16_SPLIT, PREC_FP16_SPLIT8)   # head + leading blocks in three passes, the rest with bf6 / e4m3 terms
PREC_NAMES = {PREC_FP16X3: 'fp16x3', PREC_FP16X1: 'fp16x1', PREC_FP16_FP8: 'fp16_fp8', PREC_FP16_E4M3: 'fp16_e4m3',
              PREC_FP16X3_ASM: 'fp16x3_asm', PREC_FP16_SPLIT: 'fp16_split', PREC_FP16_SPLIT8: 'fp16_split8'}


def _dev(device=None):
    if not torch.cuda.is_available():
        raise R2LError('no HIP device visible to torch: the R2L path has no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def watch_diff(got, ref, owner=None):
    """What every watch compares two renders of the same rays with.  A ray with a NaN in its embedding renders as NaN in every mode
    (DESIGN.md §4), so a NaN on both sides is agreement, not a miss: the largest |got - ref| over the elements that are numbers on both
    sides.  Where the NaN masks differ the result is NaN, which fails every `d <= limit`.  A sample that is NaN on both sides throughout
    compares nothing: 0.0, counted in `owner.watch_all_nan` and said on stderr."""
    both = torch.isnan(got) & torch.isnan(ref)
    if got.numel() == 0:
        return 0.0
    d = float(torch.where(both, torch.zeros_like(got), (got - ref).abs()).max())     # a NaN on one side only stays one
    if d == 0.0 and bool(both.all()):
        if owner is not None:
            owner.watch_all_nan = getattr(owner, 'watch_all_nan', 0) + 1
        print(f'[precision] watch: all {got.numel()} sampled values are NaN in both renders (non-finite rays): nothing compared, '
              f'difference 0', file=sys.stderr)
    return d


def _c2w_host(c2w):
    c = torch.as_tensor(c2w).detach().to('cpu', torch.float32)
    if c.shape[-2:] == (4, 4):
        c = c[..., :3, :4]
    if c.shape != (3, 4):
        raise R2LError(f'c2w must be [3,4] (or [4,4]); got {tuple(c.shape)}')
    return c.contiguous()


class R2LEngine:
    """One r2l_ctx: geometry + weights + launches (include/r2l_hip.h)."""

    def __init__(self, H, W, focal, near=2., far=6., n_sample=16, L=10, width=256, n_block=43,
                 use_residual=True, precision=PREC_FP16X3, device=None, z_vals=None, res_scale=1.0, act='relu', inact='relu',
                 outact='none', body_arch='resmlp'):
        """res_scale: ResMLP's `--trial.res_scale` (model/nerf_raybased.py:461: x = body(x).mul(res_scale) + x).  The kernels
        compute x += W2 h + b2; the factor is folded into W2 and b2 when the weights are loaded (exact for powers of two, one
        fp32 rounding per weight otherwise: far inside the 1e-4 contract).
        act / inact / outact: args.act (behind the head layer), trial.inact (inside a ResMLP block), trial.outact (behind it) of the
        reference (model/nerf_raybased.py:468-476, 497-522): 'relu' | 'lrelu' | 'none'.  Other than relu / relu / none renders in
        the compiler-scheduled modes only; the generated ones refuse (r2l_set_activations).
        body_arch: 'resmlp' (the README's), or 'mlp' (model/nerf_raybased.py:515-518: 2 n_block plain Linear + act layers, state_dict
        keys body.{0,2,4,...}; two consecutive layers ride in one block without its residual; inact / outact / res_scale do not
        apply) -- compiler-scheduled modes only."""
        self.device = _dev(device)
        self.res_scale = float(res_scale)
        if body_arch not in ('resmlp', 'mlp'):
            raise R2LError(f'body_arch={body_arch!r}: resmlp or mlp (model/nerf_raybased.py:499-518)')
        self.body_arch = body_arch
        if body_arch == 'mlp':
            inact = outact = act          # every layer is Linear + act
            self.res_scale = 1.0
        self.acts = tuple(self.ACT_SLOPES[str(a).lower()] if str(a).lower() in self.ACT_SLOPES else self._bad_act(a) for a in (act, inact, outact))
        self.H, self.W, self.focal = int(H), int(W), float(focal)
        self.n_block = int(n_block)
        self.use_residual_flag = bool(use_residual)
        self._watch_eng = self._watch_state = None
        self._ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().r2l_create(C.byref(self._ctx), self.H, self.W, self.focal, float(near), float(far),
                                   int(n_sample), int(L), int(width), self.n_block, int(bool(use_residual)),
                                   int(precision)))
        if self.acts != (0.0, 0.0, 1.0) or body_arch == 'mlp':
            check(lib().r2l_set_network_form(self._ctx, *self.acts, int(body_arch == 'resmlp')))
        self.precision = int(precision)
        # R2L_PREC_FP16_SPLIT: leading blocks in three passes = first block of the bf6 part (the library's default: half)
        self.split_block = self.n_block // 2 if self.precision in TWO_PART else None
        self._loaded = False
        # model/nerf_raybased.py:88-90, evaluated with the host's torch exactly as the
        # reference does (torch.linspace's last ulp depends on the CPU vector width)
        if z_vals is None:
            t_vals = torch.linspace(0., 1., steps=int(n_sample))
            z_vals = float(near) * (1 - t_vals) + float(far) * (t_vals)
        self.set_z_vals(z_vals)

    #: get_activation (model/nerf_raybased.py:468-476) as the slope s of act(v) = max(v, s v)
    ACT_SLOPES = {'relu': 0.0, 'lrelu': 0.01, 'none': 1.0}

    @staticmethod
    def _bad_act(a):
        raise R2LError(f'activation {a!r}: the reference knows relu, lrelu and none (model/nerf_raybased.py:468-476)')

    def set_z_vals(self, z_vals):
        z = torch.as_tensor(z_vals).detach().to('cpu', torch.float32).contiguous()
        check(lib().r2l_set_z_vals(self._ctx, C.c_void_p(z.data_ptr()), z.numel()))
        self.z_vals = z

    def close(self):
        if getattr(self, '_watch_eng', None) is not None:
            self._watch_eng.close()
            self._watch_eng = None
        if getattr(self, '_ctx', None) and self._ctx.value and _lib._lib is not None:
            lib().r2l_destroy(self._ctx)
            self._ctx = C.c_void_p()

    __del__ = close

    # -- weights --------------------------------------------------------------------
    @staticmethod
    def state_names(n_block):
        names = ['head.0.weight', 'head.0.bias']
        for i in range(n_block):
            for j in (0, 2):
                names += [f'body.{i}.body.{j}.weight', f'body.{i}.body.{j}.bias']
        return names + ['tail.0.weight', 'tail.0.bias']

    def load_state_dict(self, state_dict):
        """state_dict of the reference's NeRF_v3_2 (``module.`` prefixes tolerated,
        utils/run_nerf_raybased_helpers.py:408-425)."""
        sd = {(k[7:] if k.startswith('module.') else k): v for k, v in state_dict.items()}
        if self.body_arch == 'mlp':       # nn.Sequential(Linear, act, Linear, act, ...): Linear k at index 2 k; pairs -> blocks
            sd = dict(sd)
            for i in range(self.n_block):
                for j, src in ((0, 4 * i), (2, 4 * i + 2)):
                    for kind in ('weight', 'bias'):
                        if f'body.{src}.{kind}' in sd:
                            sd[f'body.{i}.body.{j}.{kind}'] = sd[f'body.{src}.{kind}']
        elif self.n_block and 'body.0.body.2.weight' not in sd and 'body.0.body.1.weight' in sd:
            # trial.inact = none: ResMLP's nn.Sequential holds no activation module, its second Linear is body.{i}.body.1
            # (model/nerf_raybased.py:450-454)
            sd = dict(sd)
            for i in range(self.n_block):
                for kind in ('weight', 'bias'):
                    if f'body.{i}.body.1.{kind}' in sd:
                        sd[f'body.{i}.body.2.{kind}'] = sd[f'body.{i}.body.1.{kind}']
        names = self.state_names(self.n_block)
        missing = [n for n in names if n not in sd]
        if missing:
            raise R2LError(f'state_dict lacks {len(missing)} tensors, e.g. {missing[:3]}')
        # a checkpoint with more body layers than this engine was built for must not render with the rest silently dropped
        # (--trial.n_block with the mlp body): body.{k}... with k beyond what the plan consumes is an error
        n_src = 4 * self.n_block if self.body_arch == 'mlp' else self.n_block
        extra = sorted(k for k in sd if k.startswith('body.') and k.split('.')[1].isdigit() and int(k.split('.')[1]) >= n_src)
        if extra:
            raise R2LError(f'state_dict has body layers this engine (n_block={self.n_block}, body_arch={self.body_arch}) does not '
                           f'consume, e.g. {extra[:3]}: netdepth / trial.n_block do not match the checkpoint')
        shapes = {'head.0.weight': (256, 1008), 'tail.0.weight': (3, 256), 'tail.0.bias': (3,)}
        for n in names:
            want = shapes.get(n, (256, 256) if n.endswith('weight') else (256,))
            if tuple(sd[n].shape) != want:
                raise R2LError(f'{n}: shape {tuple(sd[n].shape)} != {want}')
        if self.res_scale != 1.0:      # (W2 h + b2) s + x = (s W2) h + s b2 + x
            sd = dict(sd)
            for i in range(self.n_block):
                for k in (f'body.{i}.body.2.weight', f'body.{i}.body.2.bias'):
                    sd[k] = sd[k].detach().to('cpu', torch.float32) * self.res_scale
        keep, arr = _lib.host_ptrs([sd[n] for n in names])
        # a load the library refuses (weights the mode cannot pack) leaves the context unloaded (include/r2l_hip.h): so does this side, and
        # the watch context, which holds the previous weights, goes with them
        self._loaded = False
        self._watch_state = None
        if getattr(self, '_watch_eng', None) is not None:
            self._watch_eng.close()
        self._watch_eng = None
        with torch.cuda.device(self.device):
            check(lib().r2l_load_weights(self._ctx, arr, len(keep)))
        self._loaded = True
        # a snapshot (float32 CPU clones, 23 MB for the 88-layer student), not references: the watch context is built lazily, and the caller
        # may have changed or freed its tensors by then
        self._watch_state = {n: t.clone() for n, t in zip(names, keep)}
        return self

    def set_precision(self, precision):
        with torch.cuda.device(self.device):
            check(lib().r2l_set_precision(self._ctx, int(precision)))
        self.precision = int(precision)
        if self.precision in TWO_PART and self.split_block is None:
            self.set_split_block(self.n_block // 2)       # the library's default, said explicitly so that both sides agree

    # -- rendering ------------------------------------------------------------------
    def _rows(self, rows):
        r0, r1 = (0, self.H) if rows is None else (int(rows[0]), int(rows[1]))
        return r0, r1

    def render(self, c2w, rows=None, out=None):
        """rgb [rows*W, 3] for one pose given on the host (c2w [3,4] or [4,4])."""
        r0, r1 = self._rows(rows)
        c = _c2w_host(c2w)
        n = (r1 - r0) * self.W
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().r2l_render(self._ctx, C.c_void_p(c.data_ptr()), 0, 1, r0, r1, dptr(out), current_stream()))
        return out

    def render_batch(self, c2w_dev, rows=None, out=None):
        """rgb [P, rows*W, 3] for P poses resident on the device ([P,3,4] f32): one launch."""
        r0, r1 = self._rows(rows)
        if c2w_dev.dim() == 2:
            c2w_dev = c2w_dev[None]
        if c2w_dev.shape[-2:] != (3, 4):
            raise R2LError(f'c2w_dev must be [P,3,4]; got {tuple(c2w_dev.shape)}')
        P = c2w_dev.shape[0]
        n = (r1 - r0) * self.W
        if out is None:
            out = torch.empty((P, n, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().r2l_render(self._ctx, dptr(c2w_dev), 1, P, r0, r1, dptr(out), current_stream()))
        return out

    def render_rays(self, rays_o, rays_d, out=None):
        """Given-rays path (main.py:220-230): rays_o, rays_d [n,3] device f32 -> rgb [n,3]."""
        n = rays_o.shape[0]
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().r2l_render_rays(self._ctx, dptr(rays_o), dptr(rays_d), n, dptr(out), current_stream()))
        return out

    def sample_embed(self, c2w, rows=None, want_pts=True, want_emb=True):
        r0, r1 = self._rows(rows)
        c = _c2w_host(c2w)
        n = (r1 - r0) * self.W
        pts = torch.empty((n, 48), dtype=torch.float32, device=self.device) if want_pts else None
        emb = torch.empty((n, 1008), dtype=torch.float32, device=self.device) if want_emb else None
        with torch.cuda.device(self.device):
            check(lib().r2l_sample_embed(self._ctx, C.c_void_p(c.data_ptr()), r0, r1, dptr(pts), dptr(emb),
                                         current_stream()))
        return pts, emb

    def debug_body(self, x_in):
        """The hand-scheduled body kernel alone (PREC_FP16_FP8): x_in [n_tiles, 4, 32, 64, 4] f32 device
        tensor in the register-image layout -> body(x_in), same layout (parity tests)."""
        if x_in.dim() != 5 or tuple(x_in.shape[1:]) != (4, 32, 64, 4):
            raise R2LError(f'x_in must be [n_tiles,4,32,64,4]; got {tuple(x_in.shape)}')
        out = torch.empty_like(x_in)
        with torch.cuda.device(self.device):
            check(lib().r2l_debug_body(self._ctx, dptr(x_in), dptr(out), x_in.shape[0], current_stream()))
        return out

    def act_exponents(self):
        """The 2 n_block + 1 bf6 activation exponents the FP16_FP8 body kernel uses (x_0, h_0, x_1, ...): measured by
        the first render after load_state_dict on that render's own rays, or set by set_act_exponents."""
        n = 2 * self.n_block + 1
        buf = (C.c_int * n)()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            check(lib().r2l_get_act_exponents(self._ctx, buf, n))
        return list(buf)

    def set_act_exponents(self, exps=None):
        """Fix the exponents (list of 2 n_block + 1 ints), or None: measure them again on the next render."""
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            if exps is None:
                check(lib().r2l_set_act_exponents(self._ctx, None, 0))
            else:
                arr = (C.c_int * len(exps))(*[int(e) for e in exps])
                check(lib().r2l_set_act_exponents(self._ctx, arr, len(exps)))
        return self

    # -- range tracking (include/r2l_hip.h: r2l_range_status) ----------------------------------
    def set_guard_period(self, period):
        """0: never run the range-guard build of the body kernel; 1: every launch; k: the first launch and every k-th"""
        check(lib().r2l_set_guard_period(self._ctx, int(period)))
        self._guard_period = int(period)
        return self

    def range_status(self, reset=False):
        """dict of r2l_range_status: how far the values rendered since the last reset filled the bf6 scales in use
        (synchronises)"""
        st = _lib.RangeStatus()
        with torch.cuda.device(self.device):
            check(lib().r2l_get_range_status(self._ctx, C.byref(st), int(bool(reset))))
        return st.as_dict()

    def recalibrate(self):
        """exponents from the maxima the guarded launches (and every head launch) collected since the last reset"""
        with torch.cuda.device(self.device):
            check(lib().r2l_recalibrate(self._ctx, current_stream()))
        return self

    def calibrate_on(self, c2w=None, rays=None):
        """Measure the activation exponents on EVERY ray of a whole frame (pose `c2w`) or of the given rays
        (rays_o, rays_d): one range-guarded render (its own 1,024-ray sample gives provisional exponents, as any first
        call), then the exponents the full set of rays asks for.  Returns the exponents (synchronises)."""
        self.set_act_exponents(None)
        self.range_status(reset=True)
        period = self._guard_period
        self.set_guard_period(1)
        if rays is not None:
            self.render_rays(rays[0].contiguous().to(self.device, torch.float32), rays[1].contiguous().to(self.device, torch.float32))
        elif c2w is not None:
            self.render(c2w)
        else:
            raise R2LError('calibrate_on needs a pose or rays')
        self.recalibrate()
        self.set_guard_period(period)
        ex = self.act_exponents()
        self.stream_max = self.range_status(reset=True)['stream_max']   # largest |activation| of any operand set of those rays
        return ex

    _guard_period = 8

    #: `--precision auto`'s ladder: the largest |activation| over all operand sets (`stream_max`, measured on every ray) up to
    #: which a mode stays inside the 1e-4 rgb contract with margin.  The error of the low-precision terms is proportional to it.
    #: Measured slopes, L_inf against fp16x3 / max|a|, W256D88 at 800x800, three poses: nn.Linear-uniform weights x gain (three
    #: seeds, profiles/r03_range_sweep.txt) AND uniform / Laplace / 50 %-sparse / outlier-laden weights (five seeds each,
    #: profiles/r04_range_sweep_dists.txt): bf6 terms <= 1.02e-5 up to max|a| = 8 (outlier weights; the other families <= 8.8e-6),
    #: e4m3 terms <= 7.6e-6 (outlier weights; the others <= 6.0e-6).  With a budget of 8e-5: bf6 up to max|a| = 8 (= activation
    #: exponent 3: worst of 45 cells 6.8e-5), e4m3 up to 10 (worst cell inside 5.5e-5; at 11.45 an outlier network reads 8.7e-5, so
    #: the rung does NOT cover all of exponent 4 as it did in round 3), above: fp16x3_asm, three fp16 passes on the same generated
    #: kernels (no low-precision term, no scales, nothing to watch: 5-7e-7 against the reference golden).
    AUTO_MAX_ABS = 8.0         # fp16_fp8 (bf6 x bf6 terms, 1.5 pass-equivalents)
    AUTO_MAX_ABS_E4M3 = 10.0   # fp16_e4m3 (e4m3 x e4m3 terms, 2.0 pass-equivalents)
    AUTO_MAX_EXP = 3           # = log2(AUTO_MAX_ABS): the exponent view of the first limit (messages, bench.py)
    AUTO_MAX_EXP_E4M3 = 4      # the exponent the middle rung lies in (it covers max|a| in (8, 10] of (8, 16])
    LADDER = (PREC_FP16_FP8, PREC_FP16_E4M3, PREC_FP16X3_ASM)

    def _rung_for(self, amax, max_exp=None):
        """index into LADDER for a largest |activation| of `amax`; max_exp (tests): fp16_fp8 up to 2^max_exp, no middle rung"""
        if max_exp is not None:
            return 0 if amax <= 2.0 ** int(max_exp) else 2
        return 0 if amax <= self.AUTO_MAX_ABS else 1 if amax <= self.AUTO_MAX_ABS_E4M3 else 2

    def choose_precision(self, c2w=None, rays=None, max_exp=None):
        """`--precision auto`: the fastest mode the network's own activation ranges allow: fp16_fp8 (bf6 correction terms)
        up to max|a| = 8, fp16_e4m3 up to 10, fp16x3_asm above.  The error of the low-precision terms is relative to the residual
        stream, the contract (L_inf <= 1e-4 on rgb) is absolute, so the choice needs the ranges of THESE weights:
        `calibrate_on` measures them on every ray of the frame of pose `c2w` (or of the given `rays` = (rays_o, rays_d); `c2w` may be a
        list of poses: ranges from the first, the two measurements below over all).
        The rung the limits name is then verified against three passes on the probe frame (AUTO_VERIFY), and networks beyond the limits
        -- or failing that check -- get a measured split rung (choose_split).
        `max_exp` overrides fp16_fp8's limit and disables the middle step and both measurements (tests).  What is rendered afterwards stays
        watched (range_status / `check_ranges`, which applies the same limits to what it sees).  Synchronous, once per weight load.
        Weights the generated kernels cannot pack (a layer with max|w| outside 2^-12 .. 2^6) get fp16x3, the compiler-scheduled
        mode with per-layer scales: ('fp16x3', None), the library's message in `auto_note`.
        Returns (name of the chosen precision, largest exponent); `stream_max` holds the largest |activation|."""
        try:
            self.set_precision(PREC_FP16_FP8)
        except R2LError as e:
            # a layer whose max|w| is outside 2^-12 .. 2^6: the generated kernels' fp16 + residual split of the weights does not
            # cover it (r2l_capi.hip pack_body_v3 / pack_head_v1 refuse); the compiler-scheduled mode scales every layer
            self.set_precision(PREC_FP16X3)
            self._auto = None
            self.auto_note = str(e)
            return 'fp16x3', None
        if self.n_block == 0:
            return 'fp16_fp8', 0
        # a list of poses (frontend.render_path: first, middle, last of the path): ranges from the first, as every first render does;
        # the verification and the split measurement below on all of them
        top = max(self.calibrate_on(c2w=c2w[0] if isinstance(c2w, (list, tuple)) else c2w, rays=rays))
        self._auto = (max_exp,)
        mode = self.LADDER[self._rung_for(self.stream_max, max_exp)]
        self.split_block = None
        self.auto_verify = self.auto_split = None
        if mode != PREC_FP16X3_ASM and max_exp is None and self.AUTO_VERIFY:
            # the limits come from i.i.d. weight families; a trained network amplifies what its early layers get wrong (the trained-like
            # student scaled to max|a| = 4 -- a ReLU network is positively homogeneous, the function and its rgb error are the same -- is
            # 1.3e-4 off in fp16_fp8): the rung the limits name is rendered against three passes on every ray of the probe frame
            if mode != PREC_FP16_FP8:
                self.set_precision(mode)
            got = self._probe_render(c2w, rays).clone()
            self.set_precision(PREC_FP16X3_ASM)
            self.auto_verify = watch_diff(got, self._probe_render(c2w, rays), self)
            if self.auto_verify <= self.AUTO_VERIFY_MAX_DIFF:
                self.set_precision(mode)
                self.range_status(reset=True)
                return PREC_NAMES[mode], top
            mode = PREC_FP16X3_ASM               # ... a miss (or NaN): the measured rungs
        if mode == PREC_FP16X3_ASM and max_exp is None and self.AUTO_SPLIT:
            split, diff = self.choose_split(c2w=c2w, rays=rays)
            if split is not None:
                return PREC_NAMES[self.precision], top
        if mode != PREC_FP16_FP8:
            self.set_precision(mode)          # the exponents travel with a switch between the two split modes
            if mode in SPLIT_MODES:
                self.range_status(reset=True)
        return PREC_NAMES[mode], top

    #: the split rungs (round 5, from the trained-like fixture: profiles/r05_split_time.txt).  A trained ResMLP lands beyond the activation
    #: limits of fp16_fp8 / fp16_e4m3 (max|a| 126 where they admit 8 / 10-ish), and measured on that network the limits are right about
    #: the whole-network modes: fp16_fp8 is 1.3-1.5e-4 from three passes (35 of 640,000 rays beyond 1e-4).  But the error is not spread
    #: evenly: the bf6-term HEAD launch alone costs 9e-5 (its output feeds every block), and of the body blocks the early ones cost
    #: most, because everything behind a block amplifies what it got wrong.  R2L_PREC_FP16_SPLIT / _SPLIT8 therefore keep the head launch
    #: and the first `split` blocks in three passes and render the rest with bf6 / e4m3 terms; when the limits send a network to the last
    #: rung, `auto` MEASURES: every ray of the probe frame, rendered with a candidate split and with three passes everywhere
    #: (split = n_block, bit for bit fp16x3_asm), bisecting for the smallest split within AUTO_SPLIT_MAX_DIFF -- for both formats, and
    #: takes the cheaper of the two results by BLOCK_COST (the fixture: e4m3 terms from block 0 on, 11.1 ms per 800 x 800 frame, against
    #: bf6 terms from block 21 on, 12.5 ms; its second variant: bf6 from block 9, 10.9 ms).  The limit keeps a factor of two to the
    #: contract for the poses the probe did not see (measured: up to 1.4 x the probe frame's maximum; watched: spot_check_split against
    #: SPLIT_WATCH_MAX_DIFF) and the 4e-6 between three passes and fp32.
    AUTO_SPLIT = True
    #: the whole-network rungs the activation limits name are verified once per weight load: rgb of the probe frame against three passes
    #: everywhere (fp16x3_asm); beyond AUTO_VERIFY_MAX_DIFF the network goes to the measured split rungs whatever its activations are
    AUTO_VERIFY = True
    AUTO_VERIFY_MAX_DIFF = 7e-5
    AUTO_SPLIT_MAX_DIFF = 5e-5
    SPLIT_WATCH_MAX_DIFF = 7e-5
    SPLIT_WATCH_RAYS = 65536
    #: choose_split takes a split that passes within this fraction of the limit outright; between that and the limit only when the next
    #: split passes too (the maximum over rays is noisy at the 1e-5 level)
    SPLIT_MARGIN = 0.8
    #: a split that would save less than this fraction of the three-pass body's time is not worth two launches and a watch: fp16x3_asm
    SPLIT_MIN_GAIN = 0.05
    #: the whole-network rungs under watch (round 6): fp16_fp8 / fp16_e4m3 chosen by `auto` were verified against three passes on the
    #: probe frames only (AUTO_VERIFY); afterwards check_ranges watches activation RANGE, and range does not predict error (the trained-like
    #: student scaled to max|a| = 3.9 is 1.35e-4 off in fp16_fp8).  spot_check_rgb renders WHOLE_WATCH_RAYS of a batch's rays again in a
    #: second context that holds the same weights in three passes (fp16x3_asm: no switch of this context, no re-pack) and compares rgb
    #: under the split rungs' limit; a miss sends the network to the measured split rungs (step_down_whole).  One tile round of both
    #: kernels ~ 1.5 ms: every WHOLE_WATCH_EVERY-th batch (frontend.render_path) that is < 1 % of the loop.
    WHOLE_WATCH_RAYS = 32768
    WHOLE_WATCH_EVERY = 16
    WHOLE_WATCH_MAX_DIFF = 7e-5
    #: measured time of one ResMLP block at 800 x 800 in units of the bf6 kernel's (profiles/r05_split_time.txt: frame time over the split,
    #: 0.129 ms per block moved from bf6 terms to three passes, 0.099 from e4m3 terms; bf6 0.205 ms, e4m3 0.235, three passes 0.334)
    BLOCK_COST = {PREC_FP16_SPLIT: 1.0, PREC_FP16_SPLIT8: 1.15, PREC_FP16X3_ASM: 1.63}

    @property
    def precision_name(self):
        return PREC_NAMES[self.precision]

    def set_split_block(self, split):
        """R2L_PREC_FP16_SPLIT / _SPLIT8: the number of leading blocks in three passes = first block of the bf6 / e4m3 part
        (0 .. n_block); takes effect at the next render"""
        with torch.cuda.device(self.device):
            check(lib().r2l_set_split_block(self._ctx, int(split)))
        self.split_block = int(split)

    def _probe_render(self, c2w, rays):
        """the probe frame(s) of choose_precision / choose_split: the given rays, one pose, or a list of poses (rendered one after the
        other: the decisions are taken on the largest difference over all of them)"""
        if rays is not None:
            return self.render_rays(rays[0].contiguous().to(self.device, torch.float32), rays[1].contiguous().to(self.device, torch.float32))
        if isinstance(c2w, (list, tuple)):
            return torch.cat([self.render(p).clone() for p in c2w], 0)
        return self.render(c2w)

    def split_cost(self, mode, split):
        """body time of a two-part render in units of one bf6 block (BLOCK_COST)"""
        return self.BLOCK_COST[PREC_FP16X3_ASM] * split + self.BLOCK_COST[mode] * (self.n_block - split)

    def choose_split(self, c2w=None, rays=None, max_diff=None, modes=TWO_PART):
        """Per format of `modes` (bf6 terms, e4m3 terms) the smallest split whose render of the probe frame is within `max_diff`
        (default AUTO_SPLIT_MAX_DIFF) of three passes everywhere, by bisection (the difference falls with the split, up to the noise of
        a maximum over rays); leaves the context in the cheaper of the two (split_cost) with its split, or in fp16x3_asm when that
        would save less than SPLIT_MIN_GAIN of the three-pass body.  Returns (split or None, its difference).  `auto_split` keeps
        {mode name: {split tried: difference}}.  Called with the exponents of fp16_fp8 calibrated (choose_precision); synchronous,
        once per weight load, about a dozen frames."""
        max_diff = self.AUTO_SPLIT_MAX_DIFF if max_diff is None else float(max_diff)
        nb = self.n_block
        rend = lambda: self._probe_render(c2w, rays)
        self.auto_split, best, ref = {}, None, None
        for mode in modes:
            try:
                self.set_precision(mode)             # the calibrated exponents travel with the switch
            except R2LError as e:
                self.auto_note = str(e)
                continue
            if ref is None:
                self.set_split_block(nb)
                ref = rend().clone()
            tried = self.auto_split[PREC_NAMES[mode]] = {}

            def diff(sp):
                if sp >= nb:
                    return 0.0
                if sp not in tried:
                    self.set_split_block(sp)
                    tried[sp] = watch_diff(rend(), ref, self)
                return tried[sp]

            def ok(sp):
                # the difference is a maximum over rays and not monotone in the split at the 1e-5 level (the fixture: 5.75e-5 at 17,
                # 7.9e-5 at 20, 4.99e-5 at 22 against a limit of 5e-5): a split is taken when it passes with margin, or when the next
                # one passes as well
                d = diff(sp)
                return d <= self.SPLIT_MARGIN * max_diff or (d <= max_diff and diff(sp + 1) <= max_diff)      # NaN fails
            # everything at or above `hi` qualifies (nb: zero difference), everything below `lo` does not; no use looking above what
            # the format found so far already beats
            lo, hi = 0, nb
            if best is not None:
                x = (best[0] - self.BLOCK_COST[mode] * nb) / (self.BLOCK_COST[PREC_FP16X3_ASM] - self.BLOCK_COST[mode])
                if x <= 0:
                    continue                         # this format with no three-pass block at all costs more already
                hi = min(nb, int(math.ceil(x)) - 1)  # the largest split that would still be cheaper
                if hi < nb and not ok(hi):
                    continue
            while lo < hi:
                mid = lo if not tried else (lo + hi) // 2          # first of all: no three-pass block at all
                if ok(mid):
                    hi = mid
                else:
                    lo = mid + 1
            cost = self.split_cost(mode, hi)
            if hi < nb and (best is None or cost < best[0]):
                best = (cost, mode, hi, tried[hi])
        if best is None or best[0] > (1.0 - self.SPLIT_MIN_GAIN) * self.split_cost(PREC_FP16X3_ASM, nb):
            self.set_precision(PREC_FP16X3_ASM)
            self.split_block = None
            return None, 0.0
        _, mode, sp, d = best
        self.set_precision(mode)
        self.set_split_block(sp)
        self.range_status(reset=True)
        return sp, d

    def spot_check_split(self, rays_o, rays_d, n_rays=None):
        """the watch of the split rung: up to `n_rays` (default SPLIT_WATCH_RAYS) of the given rays, spread over the set, rendered with
        the split in use and with three passes everywhere; (ok, largest difference).  Other modes: (True, 0)."""
        if self.precision not in TWO_PART or self.split_block is None or self.split_block >= self.n_block:
            return True, 0.0
        ro, rd = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
        n = ro.shape[0]
        idx = torch.arange(0, n, max(1, n // int(n_rays or self.SPLIT_WATCH_RAYS)), device=ro.device)[:int(n_rays or self.SPLIT_WATCH_RAYS)]
        ro, rd = ro[idx].contiguous(), rd[idx].contiguous()
        sp = self.split_block
        got = self.render_rays(ro, rd).clone()
        self.set_split_block(self.n_block)
        try:
            ref = self.render_rays(ro, rd)
        finally:
            self.set_split_block(sp)
        d = watch_diff(got, ref, self)
        return d <= self.SPLIT_WATCH_MAX_DIFF, d

    def step_down_split(self):
        """after a failed spot_check_split: half of the low-precision part goes to three passes, all of it once that would save less than
        SPLIT_MIN_GAIN of the three-pass body; returns the new mode's name"""
        nb = self.n_block
        sp = (self.split_block or 0) + max(1, (nb - (self.split_block or 0) + 1) // 2)
        if sp >= nb or self.split_cost(self.precision, sp) > (1.0 - self.SPLIT_MIN_GAIN) * self.split_cost(PREC_FP16X3_ASM, nb):
            self.set_precision(PREC_FP16X3_ASM)
            self.split_block = None
            return 'fp16x3_asm'
        self.set_split_block(sp)
        return PREC_NAMES[self.precision]

    def _strided_rays(self, rays_o, rays_d, n_rays):
        ro, rd = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
        n = ro.shape[0]
        idx = torch.arange(0, n, max(1, n // int(n_rays)), device=ro.device)[:int(n_rays)]
        return ro[idx].contiguous(), rd[idx].contiguous()

    def _watch_engine(self):
        """a second context with the same weights in three fp16 passes everywhere (fp16x3_asm), sized for the watch's rays only"""
        if getattr(self, '_watch_eng', None) is None:
            rows = max(1, -(-self.WHOLE_WATCH_RAYS // self.W))
            w = R2LEngine(rows, self.W, self.focal, n_block=self.n_block, use_residual=self.use_residual_flag, precision=PREC_FP16X3_ASM,
                          device=self.device, z_vals=self.z_vals)
            w.load_state_dict(self._watch_state)
            w._watch_state = None
            self._watch_eng = w
        return self._watch_eng

    def watched_mode(self):
        """'split' / 'whole' when `auto` chose the current mode and a spot check applies to it, else None (explicit modes keep themselves;
        three passes have nothing to watch)"""
        if getattr(self, '_auto', None) is None:
            return None
        if self.precision in TWO_PART and self.split_block is not None and self.split_block < self.n_block:
            return 'split'
        if self.precision in (PREC_FP16_FP8, PREC_FP16_E4M3) and self.n_block > 0:
            return 'whole'
        return None

    def spot_check_rgb(self, rays_o, rays_d, n_rays=None):
        """the rgb watch of every rung `auto` can choose: the split rungs as spot_check_split; fp16_fp8 / fp16_e4m3: up to WHOLE_WATCH_RAYS of the
        given rays, spread over the set, rendered here and in the three-pass watch context; (ok, largest difference).  Other modes: (True, 0)."""
        if self.precision in TWO_PART:
            return self.spot_check_split(rays_o, rays_d, n_rays)
        if self.precision not in (PREC_FP16_FP8, PREC_FP16_E4M3) or self.n_block == 0:
            return True, 0.0
        ro, rd = self._strided_rays(rays_o, rays_d, n_rays or self.WHOLE_WATCH_RAYS)
        got = self.render_rays(ro, rd)
        ref = self._watch_engine().render_rays(ro, rd)
        d = watch_diff(got, ref, self)
        self.whole_watch_checks = getattr(self, 'whole_watch_checks', 0) + 1
        return d <= self.WHOLE_WATCH_MAX_DIFF, d

    def step_down_whole(self, rays_o, rays_d):
        """after a failed spot_check_rgb in fp16_fp8 / fp16_e4m3: the measured rungs -- choose_split on (a sample of) the rays that missed,
        fp16x3_asm when no split qualifies; returns the new mode's name"""
        ro, rd = self._strided_rays(rays_o, rays_d, self.SPLIT_WATCH_RAYS)
        self.range_status(reset=True)
        self.choose_split(rays=(ro, rd))
        return PREC_NAMES[self.precision]

    #: check_ranges raises the exponents when the largest value of an operand set, in units of its scale (|a| act_scale / 2^E:
    #: the calibration aims at <= 16 on the frame it saw), passes 0.9 x 28 = 25.2 -- for BOTH operand formats.  bf6 clamps at
    #: 28 (fill 1.0) and represents 16..28 as well as 8..16, so other poses may use that headroom (the 200-pose test path of
    #: the synthetic weights: up to 0.75 x 28) at no loss.  e4m3 clamps only at 448, but the error of its terms grows with |a|
    #: all the same, and the ladder admits it up to exponent 4 only: its limit is the same 1.58 x the calibrated range, not 0.9
    #: of ITS top (which would let activations grow 25-fold unnoticed).
    FILL_LIMIT = 0.9
    RAISE_AT = FILL_LIMIT * 28.0
    #: frontend.render_path / dist: how often a batch is rendered again at most (measure -> raise -> fall back -> good)
    MAX_RERENDERS = 4

    def fill_limit(self, format_top=None):
        """FILL_LIMIT in units of the operand format in use: 0.9 (bf6), 0.9 x 28 / 448 (e4m3)"""
        top = format_top or (448.0 if self.e4m3_terms else 28.0)
        return self.RAISE_AT / top

    @property
    def e4m3_terms(self):
        """the low-precision terms of the current mode are e4m3 (fp16_e4m3, fp16_split8), not bf6: the C side's e4m3_terms()"""
        return self.precision in (PREC_FP16_E4M3, PREC_FP16_SPLIT8)

    def check_ranges(self, log=None, rank_max=None, agree=None):
        """After a render in fp16_fp8 / fp16_e4m3: did the values stay inside the scales in use?  Returns None when the frame
        is good.  Otherwise the frame must be rendered AGAIN and check_ranges called again (until None; MAX_RERENDERS bounds
        the loop); the return value says why:
          'measure'   a value passed the limit (or was clamped) but only the head's running maximum exists -- 7 of 8 launches
                      at the default guard period --, so nothing is known about the other operand sets of these rays: the
                      next launch is range-guarded and measures all of them;
          a precision name: the exponents were raised from the maxima of the guarded launches (r2l_recalibrate) and values
                      WERE clamped in the frame; or (`--precision auto` only) the largest |activation| these rays produced is
                      beyond what the current rung of `choose_precision`'s ladder holds to 1e-4 -- the same limits, applied
                      to every frame -- and the context has switched (fp16_fp8 -> fp16_e4m3 -> fp16x3_asm; never back).
        Values beyond RAISE_AT that were not clamped raise the exponents for what follows and the frame stands (None).
        An explicit precision keeps its mode and says so -- with ONE exception: the two-part modes (fp16_split / fp16_split8) cannot
        re-measure their scales (their guarded launches see only the blocks behind the split, r2l_recalibrate refuses), so values beyond
        the scales send them to three passes everywhere (fp16x3_asm: always correct, slower), explicit or not, and the log says so.
        Synchronises: one stream sync + one device copy
        (r2l_get_range_status) per call, more only when it acts.
        Row-sharded runs (dist.check_ranges) pass `rank_max` (list of ints -> element-wise maximum over the ranks) and `agree` (makes the
        exponents the element-wise maximum over the ranks), so that every rank takes the same decision."""
        if self.precision not in SPLIT_MODES or self.n_block == 0:
            return None
        st = self.range_status()
        top = st['format_top']
        split = self.precision in TWO_PART
        if split and self.split_block:           # the head output is an operand of the bf6 part only when no block runs before it
            st['h0_fill'] = 0.0
            st['saturated'] = st['worst_fill'] >= 1.0
        scaled = max(st['h0_fill'], st['worst_fill']) * top
        act, clamped = scaled > self.RAISE_AT, bool(st['saturated'])
        guarded = st['guarded_launches'] > 0
        auto = getattr(self, '_auto', None)
        if split:
            # the bf6 part's scales are watched as in fp16_fp8; the ladder's activation limits are not applied: this rung was chosen
            # by measured error (choose_split) and is watched by spot_check_split.  Beyond the scales it does not raise them (its
            # guarded launches see the blocks behind the split only): three passes everywhere, nothing left to watch
            cur = want = 0
        else:
            cur = self.LADDER.index(self.precision)
            # the ladder's own limit applied to what THESE rays did (h0 of every ray; every set on the guarded launches)
            want = max(cur, self._rung_for(st['stream_max'], auto[0])) if auto is not None else cur
        if rank_max is not None:    # the ranks launch in step, so `guarded` agrees anyway; it rides along in the one all-reduce
            act, clamped, guarded, want = rank_max([act, clamped, guarded, want])
            act, clamped, guarded = bool(act), bool(clamped), bool(guarded)
        if not (act or clamped or want > cur):
            return None
        fmt = 'e4m3' if self.e4m3_terms else 'bf6'
        msg = ('[precision] activations reach %.1f in units of their %s scale (operand set %d; h0: %.1f; calibrated to <= 16, limit '
               '%.1f, clamped beyond %g)%s' % (st['worst_fill'] * top, fmt, st['worst_set'], st['h0_fill'] * top, self.RAISE_AT, top,
                                                 ': values were clamped' if clamped else ''))
        if not (act or clamped):
            # inside the scales, but larger than this rung's correction terms hold to 1e-4: down the ladder, frame rendered again
            self.range_status(reset=True)
            self.set_precision(self.LADDER[want])
            if log:
                log('[precision] largest |activation| %.2f is beyond what %s holds to 1e-4 (fp16_fp8 up to %g, fp16_e4m3 up to %g) -> %s, '
                    'frame rendered again' % (st['stream_max'], PREC_NAMES[self.LADDER[cur]], self.AUTO_MAX_ABS, self.AUTO_MAX_ABS_E4M3,
                                              PREC_NAMES[self.LADDER[want]]))
            return PREC_NAMES[self.LADDER[want]]
        if not guarded:
            self.range_status(reset=True)
            self.set_guard_period(self._guard_period)      # restarts the guard's phase: the next launch is range-guarded
            if log:
                log(msg + '; only the head output of these rays was watched: rendered again range-guarded')
            return 'measure'
        if split:
            self.range_status(reset=True)
            self.set_precision(PREC_FP16X3_ASM)
            self.split_block = None
            if log:
                log(msg + f'; {PREC_NAMES[self.precision]} cannot re-measure the blocks in front of its split -> fp16x3_asm (three passes everywhere), '
                    'frame rendered again' + ('' if auto is not None else ' [explicit precision: this is the one fallback an explicit mode has]'))
            return 'fp16x3_asm'
        before = self.act_exponents()
        self.recalibrate()
        if agree is not None:
            agree(self)
        after = self.act_exponents()
        top_e = max(after)
        self.range_status(reset=True)
        if clamped:
            # the maxima behind the new exponents come from a forward pass with clamped operands: the re-render is
            # range-guarded as well, so that the next check sees every set of the frame under the new scales
            self.set_guard_period(self._guard_period)
        if want > cur:       # never back up the ladder
            mode = self.LADDER[want]
            self.set_precision(mode)
            if log:
                log(msg + f'; exponents now up to {top_e}, largest |activation| {st["stream_max"]:.2f} -> {PREC_NAMES[mode]}, frame rendered again')
            return PREC_NAMES[mode]
        if log:
            log(msg + ('; exponents raised (up to %d)' % top_e if after != before else '; exponents unchanged') +
                (', frame rendered again' if clamped else '') +
                ('' if auto is not None else ' [explicit precision: no fallback; --precision auto has one]'))
        return PREC_NAMES[self.precision] if clamped else None

    def render_checked(self, render, log=None, check=None):
        """`render()` (any callable that launches on this context) until check_ranges has nothing left to say: the loop every
        caller of check_ranges needs (frontend.render_path, tests).  `check` replaces self.check_ranges (dist.check_ranges for
        row-sharded runs).  Returns (render()'s last result, number of extra renders)."""
        check = check or (lambda: self.check_ranges(log=log))
        out = render()
        again = 0
        while check() is not None:
            if again >= self.MAX_RERENDERS:
                raise R2LError('check_ranges asked for more than %d re-renders of one batch: activation ranges do not settle'
                               % self.MAX_RERENDERS)
            again += 1
            out = render()
        return out, again

    def _set_fused_tail(self, on):
        """parity tests: 0 = the three-launch form (body kernel writes x, r2l_tail_kernel finishes the rays)"""
        check(lib().r2l_debug_set_fused_tail(self._ctx, int(bool(on))))
        return self

    # -- introspection --------------------------------------------------------------
    @property
    def flops_per_ray(self):
        return int(lib().r2l_flops_per_ray(self._ctx))

    @property
    def kernel_flops_per_ray(self):
        """algorithmic flops per ray of the kernel the timing events bracket"""
        return int(lib().r2l_kernel_flops_per_ray(self._ctx))

    @property
    def weight_image_bytes(self):
        return int(lib().r2l_weight_image_bytes(self._ctx))

    @property
    def rays_per_tile(self):
        return int(lib().r2l_rays_per_tile(self._ctx))

    def timing(self, on=True):
        check(lib().r2l_timing_enable(self._ctx, int(on)))

    def kernel_time_ms(self, reset=True):
        tot, n = C.c_double(), C.c_int()
        check(lib().r2l_kernel_time_ms(self._ctx, C.byref(tot), C.byref(n), int(reset)))
        return tot.value, n.value


# ------------------------------------------------------------------------------------------
# reference-shaped objects
# ------------------------------------------------------------------------------------------
class LazyPoints:
    """What PointSampler.sample_test / sample_train return: the recipe for [N, 48] points."""

    def __init__(self, sampler, c2w=None, rays=None):
        self.sampler, self.c2w, self.rays = sampler, c2w, rays
        n = sampler.H * sampler.W if rays is None else rays[0].shape[0]
        self.shape = (n, sampler.n_sample * 3)

    def materialize(self):
        if self.rays is not None:
            raise R2LError('points of a given-rays bundle are only consumed by the fused kernel')
        return self.sampler._geometry_engine().sample_embed(self.c2w, want_emb=False)[0]

    tensor = property(materialize)


class LazyEmbedding:
    """What PositionalEmbedder returns for LazyPoints: the recipe for [N, 1008]."""

    def __init__(self, pts, L):
        self.pts, self.L = pts, L
        self.shape = (pts.shape[0], pts.shape[1] * (2 * L + 1))

    def materialize(self):
        if self.pts.rays is not None:
            raise R2LError('embedding of a given-rays bundle is only consumed by the fused kernel')
        if self.L != 10:
            raise R2LError(f'multires={self.L}: the stand-alone sampler + embedder kernel is built for 10 (PositionalEmbedder on a tensor takes any L)')
        return self.pts.sampler._geometry_engine().sample_embed(self.pts.c2w, want_pts=False)[1]

    tensor = property(materialize)


class PointSampler:
    """model/nerf_raybased.py:76-126.  Same constructor; sample_test(c2w) and
    sample_train(rays_o, rays_d, perturb=0) return lazy handles (see module docstring);
    sample_train with perturb > 0 (training) returns the jittered points as a tensor."""

    def __init__(self, H, W, focal, n_sample, near, far):
        if int(n_sample) < 1:
            raise R2LError(f'n_sample_per_ray={n_sample}')
        self.H, self.W, self.focal = int(H), int(W), float(focal)
        self.n_sample, self.near, self.far = int(n_sample), float(near), float(far)
        self._geo = None

    def _geometry_engine(self):
        if self.n_sample != 16:
            raise R2LError(f'n_sample_per_ray={self.n_sample}: the stand-alone sampler kernel is built for 16; the model consumes the handle '
                           f'on the generic path (generic.GenericR2L)')
        if self._geo is None:  # weight-less ctx: enough for the stand-alone K1+K2 kernels
            self._geo = R2LEngine(self.H, self.W, self.focal, self.near, self.far, n_block=0)
        return self._geo

    def sample_test(self, c2w):  # c2w: [3, 4]
        return LazyPoints(self, c2w=c2w)

    def sample_train(self, rays_o, rays_d, perturb, t_rand=None):
        if perturb > 0.:      # :117-123: jittered depths; the points are a tensor (the fused kernels sample fixed depths)
            from .train import jitter_z_vals
            ro, rd = rays_o.contiguous(), rays_d.contiguous()
            n = ro.shape[0]
            t_vals = torch.linspace(0., 1., steps=self.n_sample)      # :88-90 on the host, as the reference does
            z_vals = (self.near * (1 - t_vals) + self.far * t_vals).to(ro.device)
            pts = torch.empty((n, 3 * self.n_sample), dtype=torch.float32, device=ro.device)
            with torch.cuda.device(ro.device):
                z = jitter_z_vals(z_vals, n, t_rand)
                check(lib().r2l_sample_points(dptr(ro), dptr(rd), n, dptr(z), self.n_sample, 1, dptr(pts), current_stream()))
            return pts
        return LazyPoints(self, rays=(rays_o, rays_d))


class PositionalEmbedder:
    """model/nerf_raybased.py:191-208."""

    def __init__(self, L, include_input=True):
        if not include_input:
            raise R2LError('include_input=False is not used by the reference R2L path')
        self.L = int(L)
        self.include_input = include_input
        self.embed_dim = 2 * L + 1

    def __call__(self, x):
        if isinstance(x, LazyPoints):
            return LazyEmbedding(x, self.L)        # L != 10 / n_sample != 16: consumed by the model on the generic path
        # plain tensor [n, dim] on the device: stand-alone HIP embedder
        x = x.contiguous()
        out = torch.empty((x.shape[0], x.shape[1] * self.embed_dim), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(lib().r2l_embed(dptr(x), x.shape[0], x.shape[1], self.L, dptr(out), current_stream()))
        return out


class NeRF_v3_2:
    """model/nerf_raybased.py:480-544 for the `--trial.body_arch resmlp` family at
    netwidth 256.  ``args`` is the reference's namespace (netdepth, netwidth, use_residual,
    trial.n_block, ...).  Weights arrive through load_state_dict (the reference's
    `.tar['network_fn_state_dict']`)."""

    def __init__(self, args, input_dim, output_dim, precision=PREC_FP16X3):
        D, W = int(args.netdepth), int(args.netwidth)
        trial = getattr(args, 'trial', None)
        if output_dim != 3:
            raise R2LError(f'unsupported R2L output_dim={output_dim}')
        if getattr(args, 'linear_tail', False):
            raise R2LError('linear_tail: the reference builds Linear(input_dim, 3) on the body output and cannot run it either')
        self.body_arch = 'mlp' if trial is None else getattr(trial, 'body_arch', 'resmlp')
        if self.body_arch not in ('resmlp', 'mlp'):
            raise R2LError('--trial.body_arch resmlp or mlp')
        # shapes the fused kernels are not built for run on the generic fp32 layer path (generic.GenericR2L), fed by the same handles
        self._generic = (W != 256 or input_dim != 1008 or bool(getattr(args, 'layerwise_netwidths', ''))
                         or (self.body_arch == 'resmlp' and int(getattr(trial, 'n_learnable', 2)) != 2)
                         or (self.body_arch == 'mlp' and ((D - 2) % 2 or D < 4)))
        self._args = args
        self.res_scale = float(getattr(trial, 'res_scale', 1.))
        self.acts = (getattr(args, 'act', 'relu'), getattr(trial, 'inact', 'relu'), getattr(trial, 'outact', 'none'))
        # trial.n_block counts ResMLP blocks only (model/nerf_raybased.py:503-514); the mlp body always has netdepth - 2 layers (:515-518)
        n_block = int(getattr(trial, 'n_block', -1)) if self.body_arch == 'resmlp' else -1
        self.n_block = n_block if n_block > 0 else (D - 2) // 2
        self.use_residual = bool(getattr(args, 'use_residual', False))
        self.input_dim = input_dim
        self.precision = precision
        self._state = None
        self._engines = {}

    def load_state_dict(self, state_dict):
        self._state = {k: v.detach().to('cpu', torch.float32) for k, v in state_dict.items()}
        for eng in self._engines.values():
            eng.load_state_dict(self._state)
        return self

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def engine_for(self, sampler):
        key = (sampler.H, sampler.W, sampler.focal, sampler.near, sampler.far)
        eng = self._engines.get(key)
        if eng is None:
            if self._state is None:
                raise R2LError('NeRF_v3_2 called before load_state_dict')
            if self._generic:
                from .generic import GenericR2L
                a, per = self._args, 3 * sampler.n_sample
                if self.input_dim % per or (self.input_dim // per) % 2 == 0:
                    raise R2LError(f'input_dim={self.input_dim} is not 3 x n_sample x (2 L + 1) for n_sample={sampler.n_sample}')
                t = getattr(a, 'trial', None)
                eng = GenericR2L(sampler.H, sampler.W, sampler.focal, sampler.near, sampler.far, n_sample=sampler.n_sample,
                                 L=(self.input_dim // per - 1) // 2, netdepth=a.netdepth, netwidth=a.netwidth,
                                 layerwise_netwidths=getattr(a, 'layerwise_netwidths', ''), act=getattr(a, 'act', 'relu'),
                                 use_residual=self.use_residual, trial=None if t is None else vars(t) if hasattr(t, '__dict__') else dict(t))
                eng.load_state_dict(self._state)
                self._engines[key] = eng
                return eng
            eng = R2LEngine(sampler.H, sampler.W, sampler.focal, sampler.near, sampler.far,
                            n_block=self.n_block, use_residual=self.use_residual, precision=self.precision,
                            res_scale=self.res_scale, act=self.acts[0], inact=self.acts[1], outact=self.acts[2],
                            body_arch=self.body_arch)
            eng.load_state_dict(self._state)
            self._engines[key] = eng
        return eng

    def __call__(self, x):
        if not isinstance(x, LazyEmbedding):
            raise R2LError('the HIP NeRF_v3_2 consumes positional_embedder(point_sampler.sample_*(...)) '
                           'handles; pre-materialised [N,1008] inputs have no kernel (the embedding never '
                           'touches HBM in the fused path)')
        pts = x.pts
        if x.shape[1] != self.input_dim:
            raise R2LError(f'embedded input has {x.shape[1]} features, the network takes {self.input_dim}')
        eng = self.engine_for(pts.sampler)
        if pts.rays is not None:
            return eng.render_rays(pts.rays[0].contiguous(), pts.rays[1].contiguous())
        c2w = pts.c2w
        if torch.is_tensor(c2w) and c2w.is_cuda:
            return eng.render_batch(c2w[:3, :4].contiguous()[None])[0]
        return eng.render(c2w)

    forward = __call__


def render_func(model, pose, point_sampler, positional_embedder):
    """main.py:401-404 (the reference's --benchmark unit of work)."""
    with torch.no_grad():
        return model(positional_embedder(point_sampler.sample_test(pose)))

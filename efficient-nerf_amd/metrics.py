"""Image metrics of the reference's test report (`[TEST] TestPSNR .. TestSSIM ..`,
main.py:331-335, 384-391): PSNR from the MSE (helpers:18-20) and the Gaussian-window SSIM of
utils/ssim_torch.py, plain torch on whatever device the images live on: reporting, not hot path.  FLIP (`TestFLIP`,
main.py:371-379, utils/flip_loss.py) as the reference writes it is fourteen dense 21 x 21 convolutions per frame pair: that one runs
on the library's kernels (csrc/r2l_flip.hip), one C-ABI call.  LPIPS (`TestLPIPS`, main.py:359-369; v0.1, AlexNet trunk) likewise:
csrc/r2l_lpips.hip, from pretrained weights the user points --lpips_weights at."""
import math

import torch
import torch.nn.functional as F

from .flip_taps import FLIP_PPD


def img2mse(x, y):
    return torch.mean((x - y) ** 2)


def mse2psnr(mse):
    """-10 * log(mse) / log(10)  (utils/run_nerf_raybased_helpers.py:18-20)."""
    mse = torch.as_tensor(mse)
    return -10. * torch.log(mse) / torch.log(torch.tensor([10.], device=mse.device))


def ssim_window(window_size, channel, sigma=1.5):
    """utils/ssim_torch.py:11-25: normalised 1-D Gaussian, outer product, one copy per channel."""
    g = torch.Tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
    g = (g / g.sum()).unsqueeze(1)
    w2 = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
    return w2.expand(channel, 1, window_size, window_size).contiguous()


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/ssim_torch.py:28-53, 86-94.  img1, img2: [N, C, H, W]."""
    channel = img1.shape[1]
    window = ssim_window(window_size, channel).to(img1.device).type_as(img1)
    pad = window_size // 2
    mu1 = F.conv2d(img1, window, padding=pad, groups=channel)
    mu2 = F.conv2d(img2, window, padding=pad, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=pad, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=pad, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=pad, groups=channel) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


def ssim_hwc(img, ref):
    """main.py:46: ssim of two [H, W, 3] images (the reference permutes to [1, C, H, W])."""
    return ssim(img.permute(2, 0, 1).unsqueeze(0), ref.permute(2, 0, 1).unsqueeze(0))


def _rescale_constants(x):
    """(lo, mul, add) of main.py:361-363's rescale(x, -1, 1) = (2 / (max - min)) * (x - min) + (-1) over the whole stack, each in
    float32 as the reference's tensors hold them"""
    lo, hi = torch.aminmax(x)
    return float(lo), float(2 / (hi - lo)), -1.0


def flip(a, b, pixels_per_degree=FLIP_PPD, rescale=False, return_map=False):
    """FLIP.compute_flip(a, b, pixels_per_degree) (utils/flip_loss.py:70-130) of two stacks [N, H, W, 3] of float32 frames on
    the device: the mean over all frames as a float, with return_map also the per-pixel map [N, H, W].  One r2l_flip call on the
    current stream.  rescale=True maps each stack to [-1, 1] by its own minimum and maximum first, as main.py:359-379 does before
    it reports TestFLIP (a constant stack then gives nan, as the reference's does); rescale=False takes the images as they are."""
    from . import _lib
    if a.shape != b.shape or a.dim() != 4 or a.shape[-1] != 3:
        raise ValueError(f'flip: two stacks [N, H, W, 3] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}')
    if not (a.is_cuda and b.is_cuda and a.device == b.device and a.dtype == b.dtype == torch.float32):
        raise ValueError('flip: float32 tensors on one GPU')
    a, b = a.contiguous(), b.contiguous()
    n, H, W = (int(v) for v in a.shape[:3])
    L = _lib.lib()
    with torch.cuda.device(a.device):
        need = L.r2l_flip_workspace_floats(H, W, float(pixels_per_degree))
        if need < 0:
            _lib.check(int(need))
        ca, cb = (_rescale_constants(a), _rescale_constants(b)) if rescale and n else ((0.0, 1.0, 0.0),) * 2
        ws = torch.empty(need, dtype=torch.float32, device=a.device)
        fmap = torch.empty((n, H, W), dtype=torch.float32, device=a.device) if return_map else None
        means = torch.empty(n, dtype=torch.float32, device=a.device)
        _lib.check(L.r2l_flip(_lib.dptr(a), _lib.dptr(b), n, H, W, *ca, *cb, float(pixels_per_degree), _lib.dptr(fmap), _lib.dptr(means),
                              _lib.dptr(ws), need, _lib.current_stream()))
    mean = float(means.double().mean()) if n else float('nan')      # frames of one size: the mean of all pixels
    return (mean, fmap) if return_map else mean


# ---- LPIPS (v0.1, AlexNet trunk): TestLPIPS of main.py:359-369, on the library's kernels (csrc/r2l_lpips.hip) ----
LPIPS_CONVS = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))      # torchvision features 0, 3, 6, 8, 10
_LPIPS_TRUNK = (('slice1.0', 'features.0'), ('slice2.3', 'features.3'), ('slice3.6', 'features.6'), ('slice4.8', 'features.8'),
                ('slice5.10', 'features.10'))


def _read_state_dict(path):
    from ._lib import R2LError
    from .frontend import _pickle_mod, strip_module_prefix
    try:
        sd = torch.load(path, map_location='cpu', pickle_module=_pickle_mod, weights_only=False)
    except Exception as e:
        raise R2LError(f'--lpips_weights: cannot read "{path}": {type(e).__name__}: {e}'.splitlines()[0]) from e
    for inner in ('state_dict', 'model_state_dict'):
        if isinstance(sd, dict) and isinstance(sd.get(inner), dict):
            sd = sd[inner]
    if not isinstance(sd, dict):
        raise R2LError(f'--lpips_weights: "{path}" holds a {type(sd).__name__}, expected a state_dict')
    return {k: v for k, v in strip_module_prefix(sd).items() if torch.is_tensor(v)}


def load_lpips_weights(spec):
    """The 15 float32 CPU tensors r2l_lpips_create takes (5 conv weights [out, in, kh, kw], 5 biases, 5 lin vectors [C]) from
    `PATH` or `PATH_A:PATH_B`, read through the front end's tolerant checkpoint reader (`module.` prefixes are dropped).  Either one
    LPIPS state_dict (trunk keys ending in slice1.0 / slice2.3 / slice3.6 / slice4.8 / slice5.10 + .weight / .bias, lin keys
    lin{k}.model.1.weight or lins.{k}.model.1.weight of shape [1, C, 1, 1]) or torchvision's AlexNet state_dict
    (features.{0,3,6,8,10}.{weight,bias}) together with the lpips package's alex.pth (lin{k}.model.1.weight).  A tensor is taken by
    key suffix and shape; anything missing is one R2LError."""
    from ._lib import R2LError
    sd = {}
    for path in str(spec).split(':'):
        if path:
            sd.update(_read_state_dict(path))

    def find(what, suffixes, shape):
        hits = [k for k in sd if any(k == s or k.endswith('.' + s) for s in suffixes)]
        good = [k for k in hits if tuple(sd[k].shape) == tuple(shape)]
        if len(good) != 1:
            seen = f'{hits[0]} is {tuple(sd[hits[0]].shape)}' if hits and not good else (f'{len(good)} keys match: {good[:3]}' if good else 'no such key')
            raise R2LError(f'--lpips_weights {spec}: expected {what} {tuple(shape)} under a key ending in {" or ".join(suffixes)}, {seen}; '
                           f'the file(s) hold {len(sd)} tensors, e.g. {sorted(sd)[:4]}')
        return sd[good[0]].detach().to(torch.float32)

    weights = [find(f'conv {k + 1} weight', [f'{s}.weight' for s in _LPIPS_TRUNK[k]], LPIPS_CONVS[k]) for k in range(5)]
    biases = [find(f'conv {k + 1} bias', [f'{s}.bias' for s in _LPIPS_TRUNK[k]], LPIPS_CONVS[k][:1]) for k in range(5)]
    lins = [find(f'lin {k} weight', [f'lin{k}.model.1.weight', f'lins.{k}.model.1.weight'], (1, LPIPS_CONVS[k][0], 1, 1)).reshape(-1) for k in range(5)]
    return [t.contiguous() for t in weights + biases + lins]


def lpips_weights_from_args(args):
    """What --test_lpips needs, checked before a device is touched: None without the flag, else load_lpips_weights(--lpips_weights).
    One line (SystemExit) for --test_lpips without --lpips_weights, a --lpips_net other than alex, an unreadable or mismatched file."""
    from ._lib import R2LError
    if not getattr(args, 'test_lpips', False):
        return None
    if getattr(args, 'lpips_net', 'alex') != 'alex':
        raise SystemExit(f'--lpips_net {args.lpips_net}: --test_lpips is built for the AlexNet trunk (--lpips_net alex, the reference\'s default)')
    if not getattr(args, 'lpips_weights', ''):
        raise SystemExit('--test_lpips needs --lpips_weights PATH (one LPIPS state_dict) or PATH_A:PATH_B (torchvision\'s AlexNet state_dict and '
                         'the lpips package\'s alex.pth): the pretrained weights are not shipped')
    try:
        return load_lpips_weights(args.lpips_weights)
    except R2LError as e:
        raise SystemExit(str(e)) from e


class LPIPS:
    """LPIPS v0.1 with the AlexNet trunk on the current device: holds the library's context (the weights, copied to the device
    once).  weights: load_lpips_weights' 15 tensors.  lpips(a, b) of two stacks [N, H, W, 3] of float32 frames on that device, values
    meant to lie in [-1, 1]: the mean over the N pairs as a float, with return_layers also the per-layer distances [N, 5].  One
    r2l_lpips call on the current stream.  rescale=True maps each stack to [-1, 1] by its own minimum and maximum first, as
    main.py:359-363 does before it reports TestLPIPS; rescale=False takes the frames as they are."""

    def __init__(self, weights):
        import ctypes as C
        from . import _lib
        weights = list(weights)
        shapes = list(LPIPS_CONVS) + [s[:1] for s in LPIPS_CONVS] * 2
        if len(weights) != 15 or any(tuple(t.shape) != tuple(s) for t, s in zip(weights, shapes)):
            raise ValueError(f'LPIPS: 15 tensors of shapes {shapes}, got {[tuple(t.shape) for t in weights]}')
        self._ctx = None
        keep, arr = _lib.host_ptrs(weights)
        ctx = C.c_void_p()
        _lib.check(_lib.lib().r2l_lpips_create(C.byref(ctx), arr, len(keep)))
        self._ctx, self.device = ctx, torch.device('cuda', torch.cuda.current_device())

    def close(self):
        if getattr(self, '_ctx', None) is not None:
            from . import _lib
            _lib.lib().r2l_lpips_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __call__(self, a, b, rescale=False, return_layers=False):
        from . import _lib
        if a.shape != b.shape or a.dim() != 4 or a.shape[-1] != 3:
            raise ValueError(f'lpips: two stacks [N, H, W, 3] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}')
        if not (a.is_cuda and b.is_cuda and a.device == b.device and a.dtype == b.dtype == torch.float32):
            raise ValueError('lpips: float32 tensors on one GPU')
        if self._ctx is None or a.device != self.device:
            raise ValueError(f'lpips: the context is closed or lives on {self.device}, the frames on {a.device}')
        a, b = a.contiguous(), b.contiguous()
        n, H, W = (int(v) for v in a.shape[:3])
        L = _lib.lib()
        with torch.cuda.device(a.device):
            need = L.r2l_lpips_workspace_floats(H, W)
            if need < 0:
                _lib.check(int(need))
            ca, cb = (_rescale_constants(a), _rescale_constants(b)) if rescale and n else ((0.0, 1.0, 0.0),) * 2
            ws = torch.empty(need, dtype=torch.float32, device=a.device)
            d = torch.empty(n, dtype=torch.float32, device=a.device)
            layers = torch.empty((n, 5), dtype=torch.float32, device=a.device) if return_layers else None
            _lib.check(L.r2l_lpips(self._ctx, _lib.dptr(a), _lib.dptr(b), n, H, W, *ca, *cb, _lib.dptr(d), _lib.dptr(layers), _lib.dptr(ws), need,
                                   _lib.current_stream()))
        self.last_d = d                                                   # the pairs' own values, for tests and tools
        mean = float(d.double().mean()) if n else float('nan')
        return (mean, layers) if return_layers else mean

"""Image metrics of the reference's test report (`[TEST] TestPSNR .. TestSSIM ..`,
main.py:331-335, 384-391): PSNR from the MSE (helpers:18-20) and the Gaussian-window SSIM of
utils/ssim_torch.py, plain torch on whatever device the images live on: reporting, not hot path.  FLIP (`TestFLIP`,
main.py:371-379, utils/flip_loss.py) as the reference writes it is fourteen dense 21 x 21 convolutions per frame pair: that one runs
on the library's kernels (csrc/r2l_flip.hip), one C-ABI call."""
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

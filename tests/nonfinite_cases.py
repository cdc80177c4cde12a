"""The cases of NaN and infinity that tests/test_scan_special_gpu.py (the scan's forward) and tests/test_train_edges_gpu.py (its
backward) share: the comparisons by mask and by bits, kinds (a) .. (k) of poison on the odd rays of a launch, and the oracle's
references of each case, computed once.  No test lives here."""
import torch

from oracle import r2l_oracle as O

NAN, INF = float('nan'), float('inf')

SCAN_S = [2, 17, 64, 65, 129, 193, 256]     # one value per C of nerf_raw2outputs_kernel<C>, and its edges
SCAN_N = [1, 5, 9]
KINDS = 'abcdefghijk'
FINITE_KINDS = 'ceg'        # the reference stays finite on these (the issue's list); every other kind gives a NaN somewhere
MAPS = ['rgb', 'disp', 'acc', 'weights', 'depth']


def masks(t):
    return torch.isnan(t), t == INF, t == -INF


def same_masks(a, b):
    return a.shape == b.shape and all(torch.equal(x, y) for x, y in zip(masks(a), masks(b)))


def same_bits(a, b):
    """equal NaN masks, and equal bit patterns wherever the value is a number (so -0.0 is not 0.0)"""
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    m = ~torch.isnan(a)
    return torch.equal(a.contiguous().view(torch.int32)[m], b.contiguous().view(torch.int32)[m])


def poisoned_rays(n):
    """the odd rays: each has a clean neighbour in its workgroup (but for n = 1)"""
    return [0] if n == 1 else list(range(1, n, 2))


def poison_positions(S):
    """sample 0, 63 and 64 (the last lane of a chunk and the first of the next; with C samples per lane other lanes' edges), S - 1"""
    return sorted({p for p in (0, 63, 64, S - 1) if p < S})


def scan_case(n, S, kind, white, with_noise):
    """(clean, poisoned): two dicts raw [n,S,4], z [n,S], rd [n,3], noise [n,S] or None, g_rgb [n,3]; the poisoned one differs on the
    odd rays only.  Kind b (NaN in the noise alone) without a noise tensor has no case: None."""
    if kind == 'b' and not with_noise:
        return None
    seed = 1000 * S + 100 * n + 10 * KINDS.index(kind) + 2 * int(white) + int(with_noise)
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, S, 4, generator=g) * 2.
    raw[..., 3] = raw[..., 3] * 3. + 1.
    raw[:, [0, S - 1], 3] = raw[:, [0, S - 1], 3].abs() + 0.5        # open at both ends under any noise below: no ray is empty (acc = 0
    z = torch.sort(2. + 4. * torch.rand(n, S, generator=g), -1)[0]   # would make disp = 0 / 0 on a clean ray)
    rd = torch.randn(n, 3, generator=g)
    noise = (0.25 * torch.randn(n, S, generator=g)).clamp(-0.4, 0.4) if with_noise else None
    g_rgb = torch.randn(n, 3, generator=g)
    clean = dict(raw=raw, z=z, rd=rd, noise=noise, g_rgb=g_rgb)
    bad = {k: (None if v is None else v.clone()) for k, v in clean.items()}
    pos = poison_positions(S)
    for j, ray in enumerate(poisoned_rays(n)):
        p = pos[j % len(pos)] if n > 1 else pos[len(pos) // 2]
        if n == 5:
            p = (pos[0], pos[-1])[j % 2]
        if kind == 'a':
            bad['raw'][ray, p, 3] = NAN
        elif kind == 'b':
            bad['noise'][ray, p] = NAN
        elif kind == 'c':                       # on a positive interval: the depths are distinct, the last interval is 1e10
            bad['raw'][ray, p, 3] = INF
        elif kind == 'd':                       # a zero-length interval: not the last sample's, which is 1e10 long
            p = min(p, S - 2)
            bad['raw'][ray, p, 3] = INF
            bad['z'][ray, p + 1] = bad['z'][ray, p]
        elif kind == 'e':
            bad['raw'][ray, p, 3] = -INF
        elif kind == 'f':
            bad['raw'][ray, p, p % 3] = NAN
        elif kind == 'g':
            bad['raw'][ray, p, 0] = INF
            bad['raw'][ray, p, 1] = -INF
        elif kind == 'h':
            bad['z'][ray, p] = NAN
        elif kind == 'i':
            bad['rd'][ray] = 0.
        elif kind == 'j':
            bad['rd'][ray, p % 3] = (NAN, INF, -INF)[j % 3]
            bad['raw'][ray, p, 3] = -1.                  # a closed sample: 0 * |inf| is a NaN (open ones alone give alpha = 1, all finite)
        elif kind == 'k':
            bad['raw'][ray, p, 3] = INF
            bad['rd'][ray] = 0.
    return clean, bad


def oracle_maps(c, white, dtype):
    nz = None if c['noise'] is None else c['noise'].to(dtype)
    return O.raw2outputs(c['raw'].to(dtype), c['z'].to(dtype), c['rd'].to(dtype), white_bkgd=white, noise=nz)


_REF = {}


def scan_reference(n, S, kind, white, with_noise):
    """(clean, poisoned, the oracle's five maps of the poisoned case in float32, in float64), computed once"""
    key = (n, S, kind, white, with_noise)
    if key not in _REF:
        case = scan_case(n, S, kind, white, with_noise)
        if case is None:
            _REF[key] = None
        else:
            _REF[key] = case + (oracle_maps(case[1], white, torch.float32), oracle_maps(case[1], white, torch.float64))
    return _REF[key]


def scan_combos():
    return [(kind, white, with_noise) for kind in KINDS for white in (False, True) for with_noise in (False, True)]

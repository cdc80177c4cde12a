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


def poison_sample(bad, ray, p, kind, j=0):
    """poison `kind` of KINDS at sample p of ray `ray` of the case `bad` (scan_case's dict), in place (S >= 2 for
    kind d); j picks one of the three values of kind j"""
    S = bad['z'].shape[1]
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
        poison_sample(bad, ray, p, kind, j)
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


# ---------------------------------------------------------------------------------------------------------------------------------
# Non-finite RAYS of the fused renderers (tests/test_render_nonfinite_gpu.py, tests/test_teacher_nonfinite_gpu.py): the six poisons of
# DESIGN.md §4's table, a set of rays with some of them poisoned beside the same set with each poisoned ray replaced by a copy of the
# clean ray next to it (a duplicate adds no new maximum to any statistic of the launch), and output buffers that show what was written.
# ---------------------------------------------------------------------------------------------------------------------------------
RAY_POISONS = ('o.x=nan', 'o.y=+inf', 'd.z=nan', 'd.x=-inf', 'd=0', 'o.x=3e38')
STUDENT_NAN = (True, True, True, True, False, True)       # the student's rgb of such a ray: all three channels NaN, or finite
#: the teacher's outputs that are NaN for poison 4 (the view directions are 0 / 0, the density branch stays finite: acc = depth = 0, disp = 0 / 0);
#: for every other poison all of them are
TEACHER_KEYS = ('rgb_map', 'disp_map', 'acc_map', 'depth_map', 'rgb0', 'acc0', 'z_std')
TEACHER_NAN_D0 = {'rgb_map': True, 'disp_map': True, 'acc_map': False, 'depth_map': False, 'rgb0': True, 'acc0': False, 'z_std': False}
SENTINEL = 0x7FA5A5A5        # a NaN no kernel produces (theirs is 0x7FC00000): compared as bits
GUARD = 64                   # words behind every output that must keep the sentinel


def poison_ray(ro, rd, r, kind):
    """poison `kind` (index into RAY_POISONS) on ray r of the CPU tensors ro, rd [n, 3], in place"""
    if kind == 0:
        ro[r, 0] = NAN
    elif kind == 1:
        ro[r, 1] = INF
    elif kind == 2:
        rd[r, 2] = NAN
    elif kind == 3:
        rd[r, 0] = -INF
    elif kind == 4:
        rd[r] = 0.
    elif kind == 5:
        ro[r, 0] = 3e38
    else:
        raise ValueError(kind)


def frame_rays(H, W, n=None, theta=30., phi=-30., radius=4.):
    """the first n rays (default all) of the frame of pose_spherical(theta, phi, radius): CPU float32 [n, 3] x 2, focal"""
    focal = O.focal_from_angle(W)
    ro, rd = O.get_rays(H, W, focal, O.pose_spherical(theta, phi, radius)[:3, :4])
    ro, rd = ro.reshape(-1, 3).float()[:n].contiguous().clone(), rd.reshape(-1, 3).float()[:n].contiguous().clone()
    return ro, rd, focal


def poisoned_pair(ro, rd, positions, shift=0):
    """(bad_o, bad_d, dup_o, dup_d, kinds): position i of `positions` gets poison (i + shift) % 6 in `bad`; in `dup` it holds a copy of the
    nearest ray that is not poisoned (the one behind it, in front of it at the end of the set).  kinds: {ray: poison}."""
    n = ro.shape[0]
    bad_o, bad_d, dup_o, dup_d = ro.clone(), rd.clone(), ro.clone(), rd.clone()
    kinds = {int(r): (i + shift) % len(RAY_POISONS) for i, r in enumerate(positions)}
    for r, k in kinds.items():
        poison_ray(bad_o, bad_d, r, k)
        src = next(c for c in list(range(r + 1, n)) + list(range(r - 1, -1, -1)) if c not in kinds)
        dup_o[r], dup_d[r] = ro[src], rd[src]
    return bad_o, bad_d, dup_o, dup_d, kinds


def clean_mask(n, kinds):
    m = torch.ones(n, dtype=torch.bool)
    m[list(kinds)] = False
    return m


def sentinel_like(shape, device):
    """(out, whole): `out` of `shape`, a view of the front of the flat buffer `whole`, which is GUARD words longer; every word the sentinel"""
    numel = 1
    for s in shape:
        numel *= int(s)
    whole = torch.full((numel + GUARD,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    return whole[:numel].view(*shape), whole


def written_exactly(out, whole):
    """every word of `out` was written and none behind it"""
    bits = whole.view(torch.int32)
    n = out.numel()
    return bool((bits[:n] != SENTINEL).all()) and bool((bits[n:] == SENTINEL).all())


def no_new_inf(got, want):
    """no +-Inf in `got` where the oracle's `want` has none"""
    return not bool((torch.isinf(got) & ~torch.isinf(want)).any())


def int32_equal(a, b, rows=None):
    """bit for bit, NaN payloads included; `rows`: a boolean mask over the first dimension"""
    a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if rows is not None:
        a, b = a[rows], b[rows]
    return a.shape == b.shape and torch.equal(a, b)

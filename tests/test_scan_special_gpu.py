"""GPU: NaN and infinity through the teacher's scan kernels (csrc/nerf_kernels.hip): raw2outputs, the fused coarse scan, merge,
sort_rows, sample_pdf and row_std against torch on the CPU.

The reference is never the kernel's own formula: oracle/r2l_oracle.py (raw2outputs, sample_pdf), torch.sort and torch.std evaluated
in float32 give the NaN / +Inf / -Inf masks an output must reproduce element for element, the same functions in float64 give the
values, under the tolerances of tests/test_scan_random_gpu.py (4e-6 max(1, |ref|) for the maps, 2e-5 relative + 1e-6 for disp,
bit equality for sample_pdf under torch_sum_is_8lane() and for merge).  Poisoned rays sit at the odd indices of a launch, between
clean rays of the same four-wave workgroup, whose outputs must keep the bits they have when the poison is replaced by a finite
value; outputs go into sentinel-filled buffers whose margins must stay as they were and whose every slot must be written.

check_preconditions() runs on the CPU when the file is imported: on every case the float32 and the float64 evaluation agree on the
masks, every poisoned ray's reference is what its kind says (non-finite somewhere, or -- kinds c, e, g -- finite everywhere), and
the rows given to merge are in torch.sort's order."""
import ctypes as C

import numpy as np
import pytest
import torch

from nonfinite_cases import (FINITE_KINDS, INF, MAPS, NAN, SCAN_N, SCAN_S, poisoned_rays, same_bits, same_masks, scan_combos,
                             scan_reference)
from oracle import r2l_oracle as O
from test_scan_random_gpu import torch_sum_is_8lane

pytestmark = pytest.mark.gpu
SENT = -12345.678           # what the output buffers hold before a call: no input and no result of these cases
PAD = 32


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


# ---- the cases of merge, sort and sample_pdf ------------------------------------------------------------------------------------
MERGE_SHAPES = [(4, 4), (64, 128), (3, 253), (64, 192)]
SORT_N = [1, 2, 63, 64, 65, 128, 255, 256]
MERGE_ROWS = 9


def _grid_rows(n, k, g):
    """rows of k ascending values on a grid of eighths in [2, 6): ties inside a row and between rows"""
    return torch.sort(2. + torch.randint(0, 32, (n, k), generator=g).float() / 8., -1)[0]


def merge_case(na, nb):
    """(a, b, a_clean, b_clean, the poisoned rows): rows 1, 3, 4 hold trailing NaNs (in b, in a, in both), row 5 only NaNs, row 6
    both infinities in both inputs, row 7 zeros of both signs across the inputs, row 8 all of it; the even rows are clean"""
    g = torch.Generator().manual_seed(31 * na + nb)
    a, b = _grid_rows(MERGE_ROWS, na, g), _grid_rows(MERGE_ROWS, nb, g)
    a_clean, b_clean = a.clone(), b.clone()
    ka, kb = max(1, na // 3), max(1, nb // 3)
    b[1, nb - kb:] = NAN
    a[3, na - ka:] = NAN
    a[4, na - 1:] = NAN
    b[4, nb - kb:] = NAN
    a[5], b[5] = NAN, NAN
    for r in (6, 8):
        a[r, 0], b[r, 0] = -INF, -INF
        a[r, na - 1], b[r, nb - 1] = INF, INF
    # zeros: a row must stay ascending, so they lead it (behind -inf in row 8); 0.0 in a meets -0.0 in b and the other way round
    for r, lead in ((7, 0), (8, 1)):
        if na > lead + 1 and nb > lead + 1:
            a[r, lead], a[r, lead + 1] = 0., -0.
            b[r, lead], b[r, lead + 1] = -0., 0.
    if na > 3 and nb > 3:
        a[8, na - 2], b[8, nb - 2] = INF, INF          # ties of +inf
        a[8, na - 1], b[8, nb - 1] = NAN, NAN          # ... and the NaNs behind them
    return a, b, a_clean, b_clean, [1, 3, 4, 5, 6, 7, 8]


def merge_reference(a, b):
    return torch.sort(torch.cat([a, b], -1), dim=-1, stable=True)[0]


def sort_case(N):
    """rows of N values in random order: grid values with ties, and from row 1 on NaNs, both infinities, zeros of both signs"""
    g = torch.Generator().manual_seed(77 + N)
    x = 2. + torch.randint(0, 32, (MERGE_ROWS, N), generator=g).float() / 8.
    clean = x.clone()
    specials = [NAN, INF, -INF, 0., -0., NAN, -INF, INF]
    for r in range(1, MERGE_ROWS, 2):
        k = min(N, 1 + (r * 3) % 8)
        where = torch.randperm(N, generator=g)[:k]
        for q, w in enumerate(where):
            x[r, w] = specials[(q + r) % len(specials)]
    if N >= 2:
        x[7] = NAN                                      # a row of NaNs but for one number, in its last place
        x[7, N - 1] = 3.
    return x, clean, list(range(1, MERGE_ROWS, 2))


PDF_BINS, PDF_N = 16, 9
PDF_U = [0., 0.5, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 1.5, -0.25, NAN, INF, -INF]


def pdf_case():
    """(bins [9,16], weights [9,15], u [9,9], clean copies of the three, the poisoned rows): row 1 and row 8 the special uniforms,
    row 3 one NaN weight, row 4 one +Inf weight, row 5 all-zero weights under the special uniforms, row 6 one NaN bin"""
    g = torch.Generator().manual_seed(5)
    n = 9
    bins = torch.sort(2. + 4. * torch.rand(n, PDF_BINS, generator=g), -1)[0]
    w = torch.rand(n, PDF_BINS - 1, generator=g)
    u = torch.sort(torch.rand(n, PDF_N, generator=g), -1)[0]
    clean = (bins.clone(), w.clone(), u.clone())
    special = torch.tensor(PDF_U, dtype=torch.float32)
    u[1], u[8], u[5] = special, special, special
    w[3, 7] = NAN
    w[4, 4] = INF
    w[5] = 0.
    w[8] = 1.
    bins[6, 9] = NAN
    return bins, w, u, clean, [1, 3, 4, 5, 6, 8]


def check_preconditions():
    # the scan: float32 and float64 agree on the masks; a poisoned ray is non-finite somewhere unless its kind is c, e or g
    for S in SCAN_S:
        for n in SCAN_N:
            for kind, white, with_noise in scan_combos():
                ref = scan_reference(n, S, kind, white, with_noise)
                if ref is None:
                    continue
                clean, bad, r32, r64 = ref
                for name, a, b in zip(MAPS, r32, r64):
                    assert same_masks(a, b.float()), (n, S, kind, white, with_noise, name)
                rays = poisoned_rays(n)
                nonfinite = torch.stack([~torch.isfinite(m.reshape(n, -1)).all(-1) for m in r32]).any(0)
                if kind in FINITE_KINDS:
                    assert not nonfinite.any(), (n, S, kind)
                else:
                    assert nonfinite[rays].all(), (n, S, kind, white, with_noise)
                others = [r for r in range(n) if r not in rays]
                assert not nonfinite[others].any(), (n, S, kind)
    # merge: both inputs in torch.sort's order, the sentinel in no input, NaN or infinity in the reference of every poisoned row
    for na, nb in MERGE_SHAPES:
        a, b, ac, bc, rows = merge_case(na, nb)
        for t in (a, b, ac, bc):
            assert same_bits(torch.sort(t, dim=-1, stable=True)[0], t) and not (t == SENT).any()
        ref = merge_reference(a, b)
        assert all(not torch.isfinite(ref[r]).all() or r == 7 for r in rows) and torch.isfinite(merge_reference(ac, bc)).all()
        assert torch.isnan(ref[5]).all() and (na < 2 or nb < 2 or bool((ref[7] == 0).sum() == 4))
    for N in SORT_N:
        x, clean, rows = sort_case(N)
        assert not (x == SENT).any() and all(not torch.isfinite(x[r]).all() or (x[r] == 0).any() for r in rows)
    # sample_pdf: masks agree between float32 and float64; the special uniforms give the taps and the three NaN samples the issue lists
    bins, w, u, _, rows = pdf_case()
    s32, c32, i32 = O.sample_pdf(bins, w, PDF_N, u=u, taps=True)
    s64, c64, i64 = O.sample_pdf(bins.double(), w.double(), PDF_N, u=u.double(), taps=True)
    assert same_masks(s32, s64.float()) and same_masks(c32, c64.float())
    # the taps at u = 1 and nextafter(1, 2) hang on the last ulp of cdf[-1] (row 8: 1.0000002, tap 15; row 1: 0.99999994, tap 16;
    # float64 says 16 on both); the others do not: 0 -> 1, 1.5 -> 16, -0.25 -> 0, NaN -> 16, +Inf -> 16, -Inf -> 0
    for r in (1, 5, 8):
        assert i32[r, 0] == 1 and i32[r, 4:].tolist() == [16, 0, 16, 16, 0] == i64[r, 4:].tolist()
    assert i32[8, 2:4].tolist() == [15, 15] and i32[1, 2:4].tolist() == [16, 16]
    assert torch.isnan(s32[1, 6:]).all() and torch.isfinite(s32[1, :4]).all()
    assert torch.isnan(s32[3]).all() and torch.isnan(s32[4]).all() and torch.isfinite(s32[5, :6]).all()
    assert torch.isnan(s32[6]).any() and torch.isfinite(s32[[0, 2, 7]]).all()
    return True


check_preconditions()


# ---- 1. raw2outputs -------------------------------------------------------------------------------------------------------------
def hip_raw2outputs(L, c, white):
    """the five maps of nerf_raw2outputs_noise, each written into the middle of a sentinel-filled buffer: every slot written, the
    margins untouched"""
    n, S = c['z'].shape
    dev = {k: (None if c[k] is None else c[k].cuda().contiguous()) for k in ('raw', 'z', 'rd', 'noise')}
    sizes = [3 * n, n, n, n * S, n]
    bufs = [torch.full((PAD + k + PAD,), SENT, device='cuda') for k in sizes]
    out = [b[PAD:PAD + k] for b, k in zip(bufs, sizes)]
    _check(L, L.nerf_raw2outputs_noise(_p(dev['raw']), _p(dev['z']), _p(dev['rd']), _p(dev['noise']), n, S, int(white), *[_p(o) for o in out],
                                       _stream()))
    torch.cuda.synchronize()
    for b, k, name in zip(bufs, sizes, MAPS):
        h = b.cpu()
        assert bool((h[:PAD] == SENT).all()) and bool((h[PAD + k:] == SENT).all()), name
        assert not bool((h[PAD:PAD + k] == SENT).any()), name
    shapes = [(n, 3), (n,), (n,), (n, S), (n,)]
    return [o.cpu().view(s) for o, s in zip(out, shapes)]


@pytest.mark.parametrize('n', SCAN_N)
@pytest.mark.parametrize('S', SCAN_S)
def test_raw2outputs_non_finite_inputs(L, S, n):
    """kinds (a) .. (k) of NaN / infinity in the density, the noise, a colour, a depth or the direction, at sample 0, 63, 64 and
    S - 1, with and without a white background and a noise tensor.  Every map of nerf_raw2outputs_noise has torch-float32's NaN,
    +Inf and -Inf masks element for element and is, where finite, within 4e-6 max(1, |f64|) of the float64 oracle (disp: 2e-5
    relative + 1e-6); the clean rays keep the bits of a launch without the poison; twice the same bits."""
    for kind, white, with_noise in scan_combos():
        ref = scan_reference(n, S, kind, white, with_noise)
        if ref is None:
            continue
        clean, bad, r32, r64 = ref
        got = hip_raw2outputs(L, bad, white)
        again = hip_raw2outputs(L, bad, white)
        base = hip_raw2outputs(L, clean, white)
        others = [r for r in range(n) if r not in poisoned_rays(n)]
        for name, a, a2, b0, m32, m64 in zip(MAPS, got, again, base, r32, r64):
            tag = (name, n, S, kind, white, with_noise)
            assert same_masks(a, m32), tag
            fin = torch.isfinite(m64)
            d = (a.double() - m64).abs()[fin]
            if name == 'disp':
                assert bool((d <= 2e-5 * m64[fin].abs() + 1e-6).all()), tag
            else:
                assert bool((d <= 4e-6 * m64[fin].abs().clamp(min=1.)).all()), tag
            assert same_bits(a, a2), tag
            if n > 1:
                assert same_bits(a[others], b0[others]) and torch.isfinite(a[others]).all(), tag


# ---- 2. merge, sort, sample_pdf -------------------------------------------------------------------------------------------------
def _rows_call(L, fn, n, width, *args):
    """fn(*args, out) with out [n, width] in the middle of a sentinel-filled buffer: (out on the host, margins untouched)"""
    buf = torch.full((PAD + n * width + PAD,), SENT, device='cuda')
    out = buf[PAD:PAD + n * width]
    _check(L, fn(*args, _p(out), _stream()))
    torch.cuda.synchronize()
    h = buf.cpu()
    assert bool((h[:PAD] == SENT).all()) and bool((h[PAD + n * width:] == SENT).all())
    return h[PAD:PAD + n * width].view(n, width).clone()


@pytest.mark.parametrize('na,nb', MERGE_SHAPES)
def test_merge_sorted_with_nan_inf_and_signed_zeros(L, na, nb):
    """nerf_merge_sorted = torch.sort(cat(a, b), stable=True), bit for bit with NaNs compared by mask: trailing NaNs in b, in a, in
    both, a row of NaNs, both infinities, -0.0 against 0.0 across the inputs (a's element first on a tie).  No slot keeps the
    sentinel; the clean rows keep the bits of a launch without the poison; twice the same bits."""
    a, b, ac, bc, rows = merge_case(na, nb)
    n = a.shape[0]
    call = lambda x, y: _rows_call(L, lambda xa, xb, out, s: L.nerf_merge_sorted(xa, na, xb, nb, n, out, s), n, na + nb,
                                   _p(x), _p(y))
    ad, bd, acd, bcd = (t.cuda().contiguous() for t in (a, b, ac, bc))
    got, again, base = call(ad, bd), call(ad, bd), call(acd, bcd)
    assert not bool((got == SENT).any()), 'a slot of the output was not written'
    assert same_bits(got, merge_reference(a, b)), (na, nb)
    assert same_bits(got, again)
    clean_rows = [r for r in range(n) if r not in rows]
    assert same_bits(got[clean_rows], base[clean_rows]) and same_bits(base, merge_reference(ac, bc))


@pytest.mark.parametrize('N', SORT_N)
def test_sort_rows_with_nan_inf_ties_and_zeros(L, N):
    """nerf_sort_rows = torch.sort by value and by NaN mask (the order of -0.0 and 0.0 inside a tie is not compared): the numbers
    ascending from -inf to +inf, the NaNs behind them; every slot written; clean rows as without the poison; twice the same"""
    x, clean, rows = sort_case(N)
    n = x.shape[0]
    call = lambda t: _rows_call(L, lambda xd, out, s: L.nerf_sort_rows(xd, n, N, out, s), n, N, _p(t))
    xd, cd = x.cuda().contiguous(), clean.cuda().contiguous()
    got, again, base = call(xd), call(xd), call(cd)
    ref = torch.sort(x, -1)[0]
    assert not bool((got == SENT).any())
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), N
    m = ~torch.isnan(ref)
    assert torch.equal(got[m], ref[m]), N
    assert torch.equal(torch.isnan(got), torch.isnan(again)) and torch.equal(got[m], again[m])
    clean_rows = [r for r in range(n) if r not in rows]
    assert torch.equal(got[clean_rows], base[clean_rows]) and torch.equal(base, torch.sort(clean, -1)[0])


def _hip_sample_pdf(L, bins, w, u):
    n = bins.shape[0]
    bd, wd, ud = (t.cuda().contiguous() for t in (bins, w, u))
    sbuf = torch.full((PAD + n * PDF_N + PAD,), SENT, device='cuda')
    cbuf = torch.full((PAD + n * PDF_BINS + PAD,), SENT, device='cuda')
    ibuf = torch.full((PAD + n * PDF_N + PAD,), -77, device='cuda', dtype=torch.int32)
    s, c, i = sbuf[PAD:PAD + n * PDF_N], cbuf[PAD:PAD + n * PDF_BINS], ibuf[PAD:PAD + n * PDF_N]
    _check(L, L.nerf_sample_pdf_ex(_p(bd), _p(wd), n, PDF_BINS, _p(ud), 1, PDF_N, _p(s), _p(c), _p(i), _stream()))
    torch.cuda.synchronize()
    for buf, k, fill in ((sbuf, n * PDF_N, SENT), (cbuf, n * PDF_BINS, SENT), (ibuf, n * PDF_N, -77)):
        h = buf.cpu()
        assert bool((h[:PAD] == fill).all()) and bool((h[PAD + k:] == fill).all()) and not bool((h[PAD:PAD + k] == fill).any())
    return s.cpu().view(n, PDF_N).clone(), c.cpu().view(n, PDF_BINS).clone(), i.cpu().view(n, PDF_N).clone()


def test_sample_pdf_with_non_finite_uniforms_weights_and_bins(L):
    """nerf_sample_pdf_ex with per-ray u = {0, 0.5, 1, nextafter(1, 2), 1.5, -0.25, NaN, +Inf, -Inf}, a NaN weight, a +Inf weight,
    all-zero weights, a NaN bin: the samples have torch's masks and, where finite, torch's bits under torch_sum_is_8lane() (else the
    fallback rule of test_sample_pdf_and_merge_random); the inds tap equals torch.searchsorted(right=True) on every element, a NaN
    u included (n_bins, where `cdf <= u` gives 0), and the cdf tap torch's cdf."""
    bins, w, u, (bins_c, w_c, u_c), rows = pdf_case()
    n = bins.shape[0]
    want, cdf, inds = O.sample_pdf(bins, w, PDF_N, u=u, taps=True)
    got, gcdf, ginds = _hip_sample_pdf(L, bins, w, u)
    again = _hip_sample_pdf(L, bins, w, u)
    base = _hip_sample_pdf(L, bins_c, w_c, u_c)
    assert same_masks(got, want) and same_masks(gcdf, cdf)
    if torch_sum_is_8lane():
        assert same_bits(got, want), int((got != want).sum())
        assert same_bits(gcdf, cdf)
        assert torch.equal(ginds.long(), inds)
    else:
        fin = torch.isfinite(want)
        err = (got - want).abs()[fin]
        binw = float((bins_c[:, 1:] - bins_c[:, :-1]).max())
        assert float((err <= 2e-5).float().mean()) >= 0.98 and float(err.max()) <= binw * 1.001 + 1e-6
        special = [1, 5, 8]                                  # u away from every cdf entry: the taps cannot move by an ulp of `total`
        assert torch.equal(ginds[special].long()[:, 4:], inds[special][:, 4:])
    assert ginds[1, 6] == PDF_BINS and torch.equal(ginds[[1, 5, 8]].long()[:, 4:], inds[[1, 5, 8]][:, 4:])
    assert all(same_bits(x, y) for x, y in zip((got, gcdf, ginds.float()), (again[0], again[1], again[2].float())))
    clean_rows = [r for r in range(n) if r not in rows]
    assert same_bits(got[clean_rows], base[0][clean_rows]) and torch.equal(ginds[clean_rows], base[2][clean_rows])


# ---- 3. the fused coarse scan, and row_std, through an engine -------------------------------------------------------------------
FUSED_RAYS = 23


def _fused_inputs(eng, S0, NI, seed, poison=True):
    """23 rays of a frame, the odd ones poisoned through what a caller hands to render_rays: the coarse pass's noise (NaN at sample 0
    and at S0 - 1, +Inf on a positive and on a zero-length interval, -Inf everywhere), a coarse depth (+Inf and NaN, last in its
    row), the ray (direction 0, NaN origin, +Inf direction, +Inf density on direction 0); poison=False: the same rays without it"""
    H = eng.H
    n = FUSED_RAYS
    ro, rd = O.get_rays(H, H, eng.focal, O.pose_spherical(12., -33., 4.)[:3, :4])
    ro, rd = ro.reshape(-1, 3)[:n].float().clone(), rd.reshape(-1, 3)[:n].float().clone()
    g = torch.Generator().manual_seed(seed)
    zc = eng.z_coarse.detach().cpu().float().reshape(1, S0).expand(n, S0).clone()
    n0 = 0.7 * torch.rand(n, S0, generator=g)
    n1 = 0.7 * torch.rand(n, S0 + NI, generator=g)
    mid = S0 // 2
    if not poison:
        return ro, rd, zc, n0, n1
    n0[1, 0] = NAN
    n0[3, S0 - 1] = NAN
    n0[5, mid] = INF
    n0[7, mid] = INF
    zc[7, mid + 1] = zc[7, mid]
    n0[9] = -INF
    zc[11, S0 - 1] = INF
    rd[13] = 0.
    ro[15, 0] = NAN
    rd[17, 1] = INF
    n0[19, mid] = INF
    rd[19] = 0.
    zc[21, S0 - 1] = NAN
    return ro, rd, zc, n0, n1


def _render_ex(eng, ro, rd, zc, n0, n1):
    from efficient_nerf_amd._lib import lib, check, dptr, current_stream
    n = ro.shape[0]
    sizes = [3 * n, n, n, n]                                 # the four maps in sentinel-filled buffers: every slot written, no margin touched
    bufs = [torch.full((PAD + k + PAD,), SENT, device='cuda') for k in sizes]
    rgb, disp, acc, depth = (b[PAD:PAD + k] for b, k in zip(bufs, sizes))
    check(lib().nerf_render_rays_ex(eng._ctx, dptr(ro), dptr(rd), n, dptr(zc), None, dptr(n0), dptr(n1), dptr(rgb), dptr(disp),
                                    dptr(acc), dptr(depth), current_stream()))
    ret = {'rgb_map': rgb.view(n, 3), 'disp_map': disp, 'acc_map': acc, 'depth_map': depth}
    ret.update(eng._extras(n))
    torch.cuda.synchronize()
    for b, k in zip(bufs, sizes):
        h = b.cpu()
        assert bool((h[:PAD] == SENT).all()) and bool((h[PAD + k:] == SENT).all()) and not bool((h[PAD:PAD + k] == SENT).any())
    return {k: v.cpu().clone() for k, v in ret.items()}


@pytest.mark.parametrize('S0,NI,white', [(64, 128, True), (17, 33, False), (3, 5, True)])
def test_fused_coarse_scan_equals_the_three_launches_on_poisoned_rays(pkg, S0, NI, white):
    """The sibling of test_fused_coarse_scan_equals_the_three_launches with non-finite noise, depths and rays: every output and
    every extra of the fused launch (z_samples and the merged depths among them) has the three launches' NaN mask and bits, and on
    the twelve clean rays between the poisoned ones the bits of a launch of the same 23 rays without the poison; the four maps are
    written into sentinel-filled buffers whose margins stay.  The
    coarse maps have the masks of the float32 oracle on the coarse raw, z_samples those of the oracle's sample_pdf on the launch's
    own weights' reference, the merged depths are torch.sort(cat(z, z_samples)) wherever the caller's depths are in order, and
    z_std (nerf_row_std_kernel) has torch.std's mask: NaN on the row that holds +Inf."""
    from efficient_nerf_amd import NeRFEngine
    from efficient_nerf_amd._lib import lib, check
    H = 21
    eng = NeRFEngine(H, H, O.focal_from_angle(H), N_samples=S0, N_importance=NI, white_bkgd=white)
    eng.load_state_dicts(O.make_teacher_state(1), O.make_teacher_state(2))
    ro, rd, zc, n0, n1 = _fused_inputs(eng, S0, NI, S0 + NI)
    dev = [t.cuda().contiguous() for t in (ro, rd, zc, n0, n1)]
    outs = []
    for split in (0, 1, 0):
        check(lib().nerf_debug_set_split_scans(eng._ctx, split))
        outs.append(_render_ex(eng, *dev))
    check(lib().nerf_debug_set_split_scans(eng._ctx, 0))
    base = _render_ex(eng, *[t.cuda().contiguous() for t in _fused_inputs(eng, S0, NI, S0 + NI, poison=False)])
    raw0 = eng.run_network(0, dev[0], dev[1], dev[2]).cpu()
    eng.close()
    fused, three, again = outs
    assert set(fused) == set(three) == set(base)
    clean_rays = list(range(0, FUSED_RAYS, 2))
    for k in fused:
        assert same_bits(fused[k], three[k]), k
        assert same_bits(fused[k], again[k]), k
        # the clean rays between the poisoned ones: the bits of the launch without the poison, and finite
        assert same_bits(fused[k][clean_rays], base[k][clean_rays]) and torch.isfinite(fused[k][clean_rays]).all(), k
        assert torch.isfinite(base[k]).all(), k
    # the coarse maps against the float32 oracle on the coarse raw
    rgb0, disp0, acc0, w0, _ = O.raw2outputs(raw0, zc, rd, white_bkgd=white, noise=n0)
    for k, ref in (('rgb0', rgb0), ('disp0', disp0), ('acc0', acc0)):
        assert same_masks(fused[k], ref), k
    assert torch.isnan(fused['acc0'][[1, 3]]).all() and torch.isfinite(fused['acc0'][0::2]).all()
    # sample_pdf on the oracle's weights: the masks of z_samples
    z_mid = .5 * (zc[:, 1:] + zc[:, :-1])
    zs = O.sample_pdf(z_mid, w0[:, 1:-1], NI, det=True)
    assert same_masks(fused['z_samples'], zs)
    # the merge: where the caller's row is in torch.sort's order (every ray here but those with a repeated or non-finite depth inside)
    got_zs = fused['z_samples']
    want_all = torch.sort(torch.cat([zc, got_zs], -1), dim=-1, stable=True)[0]
    ordered = [r for r in range(FUSED_RAYS) if same_bits(torch.sort(got_zs[r], stable=True)[0], got_zs[r])]
    assert set(range(0, FUSED_RAYS, 2)) <= set(ordered) and 1 in ordered and 3 in ordered
    assert torch.equal(torch.isnan(fused['z_vals'][ordered]), torch.isnan(want_all[ordered]))
    m = ~torch.isnan(want_all[ordered])
    assert torch.equal(fused['z_vals'][ordered][m], want_all[ordered][m])
    # row_std
    std = torch.std(got_zs, dim=-1, unbiased=False)
    assert same_masks(fused['z_std'], std)
    fin = torch.isfinite(std)
    assert float((fused['z_std'][fin] - std[fin]).abs().max()) <= 1e-6
    assert not torch.isfinite(got_zs[11]).all() and torch.isnan(fused['z_std'][11])       # ray 11: a last coarse depth of +Inf
    if S0 == 64:
        assert bool((got_zs[11] == INF).any()) and not torch.isnan(got_zs[11, :NI - 1]).any()   # ... +Inf among numbers: inf - inf in the mean

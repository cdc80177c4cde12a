#!/usr/bin/env python
"""sha256 of every output of the teacher's scan entries on seeded inputs, one line per case, to compare two builds of the library bit
for bit: nerf_raw2outputs, nerf_raw2outputs_noise, nerf_train_raw2outputs_backward, nerf_sample_pdf_ex,
nerf_merge_sorted, nerf_sort_rows, and NeRFEngine.render_rays(extras=True) with the fused coarse scan and with its three launches.
The shapes are the edges of the shared device code (csrc/nerf_scan.h): one sample, the last lane of a chunk and the first of the
next for every C of the composite, a second block with one live wave, one bin interval, N across the 64-lane stride.  Every fourth
ray carries one of the poisons of tests/nonfinite_cases.py.  Every number is hashed as its bits (-0.0 is not 0.0) and every NaN as
one value, as same_bits of tests/nonfinite_cases.py compares: where two NaNs meet in a commutative operation the hardware returns the
first operand's sign and payload, the compiler orders the operands, and IEEE 754 and torch leave the choice open.  --nan-payloads
hashes the raw bytes.

    R2L_LIB_PATH=/path/to/libr2l_hip.so python tools/scan_bits.py > bits.txt
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

SCAN_S = [1, 2, 63, 64, 65, 128, 129, 192, 193, 256]
BACKWARD_S = SCAN_S + [257]
SCAN_N = [1, 5]
PDF_BINS = [2, 3, 33, 64]
PDF_N = [1, 2, 64, 65, 256]
MERGE_ROWS = 9
ENGINE = [(3, 5), (17, 33), (64, 64), (64, 128), (64, 192)]
NAN, INF = float('nan'), float('inf')


NAN_PAYLOADS = False


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        if t.is_floating_point() and not NAN_PAYLOADS:
            t = t.view(torch.int32).masked_fill(torch.isnan(t), 0x7FC00000)
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def scan_cases():
    """(tag, S, n, white, dict(raw [n,S,4], z [n,S], rd [n,3], noise [n,S] or None), g_rgb [n,3]) on the host, every fourth ray poisoned"""
    from nonfinite_cases import KINDS, poison_positions, poison_sample
    case = 0
    for S in BACKWARD_S:
        for n in SCAN_N:
            for white in (0, 1):
                for with_noise in (False, True):
                    g = torch.Generator().manual_seed(100000 + 100 * S + 10 * n + 2 * white + with_noise)
                    c = dict(raw=torch.randn(n, S, 4, generator=g) * 2., z=torch.sort(2. + 4. * torch.rand(n, S, generator=g), -1)[0],
                             rd=torch.randn(n, 3, generator=g), noise=0.25 * torch.randn(n, S, generator=g) if with_noise else None)
                    c['raw'][..., 3] = c['raw'][..., 3] * 3. + 1.
                    g_rgb = torch.randn(n, 3, generator=g)
                    pos = poison_positions(S)
                    for ray in range(0, n, 4):
                        case += 1
                        kind = KINDS[case % len(KINDS)]
                        if (kind == 'b' and not with_noise) or (kind == 'd' and S < 2):
                            kind = 'a'
                        poison_sample(c, ray, pos[case % len(pos)], kind, case)
                    yield f'S={S} n={n} white={white} noise={int(with_noise)}', S, n, white, c, g_rgb


def main():
    global NAN_PAYLOADS
    ap = argparse.ArgumentParser()
    ap.add_argument('--nan-payloads', action='store_true', help='hash the sign and payload bits of every NaN too')
    NAN_PAYLOADS = ap.parse_args().nan_payloads
    import _pkg
    _pkg.load()
    from efficient_nerf_amd import NeRFEngine
    from efficient_nerf_amd._lib import check, current_stream, lib
    from nonfinite_cases import RAY_POISONS, poison_ray
    from oracle import r2l_oracle as O
    from test_scan_special_gpu import MERGE_SHAPES, SORT_N, merge_case, sort_case
    L = lib()
    out = lambda *shape: torch.full(shape, -7., device='cuda')

    # ---- the composite and its backward
    for tag, S, n, white, c, g_rgb in scan_cases():
        raw, z, rd, gd = (t.cuda().contiguous() for t in (c['raw'], c['z'], c['rd'], g_rgb))
        nz = None if c['noise'] is None else c['noise'].cuda().contiguous()
        if S <= 256:
            maps = [out(n, 3), out(n), out(n), out(n, S), out(n)]
            if nz is None:
                check(L.nerf_raw2outputs(p(raw), p(z), p(rd), n, S, white, *[p(m) for m in maps], current_stream()))
            else:
                check(L.nerf_raw2outputs_noise(p(raw), p(z), p(rd), p(nz), n, S, white, *[p(m) for m in maps], current_stream()))
            print(f'raw2outputs {tag}: {sha(maps)}', flush=True)
        g_raw = out(n, S, 4)
        check(L.nerf_train_raw2outputs_backward(p(raw), p(z), p(rd), p(nz), n, S, white, p(gd), p(g_raw), current_stream()))
        print(f'backward {tag}: {sha([g_raw])}', flush=True)

    # ---- sample_pdf: u absent, one shared row, one row per ray
    special = [0., 0.5, 1.0, 1.5, -0.25, NAN, INF, -INF]
    for n_bins in PDF_BINS:
        for N in PDF_N:
            for u_mode in ('linspace', 'shared', 'per ray'):
                n = 9
                g = torch.Generator().manual_seed(200000 + 1000 * n_bins + N)
                bins = torch.sort(2. + 4. * torch.rand(n, n_bins, generator=g), -1)[0]
                w = torch.rand(n, n_bins - 1, generator=g)
                u = torch.sort(torch.rand(n, N, generator=g), -1)[0]
                w[0, (n_bins - 2) // 2] = NAN
                w[4] = 0.
                w[8, 0] = INF
                bins[8, n_bins - 1] = NAN
                if u_mode == 'per ray':
                    for ray in (0, 4):
                        u[ray, :] = torch.tensor([special[(k + ray) % len(special)] for k in range(N)])
                u = None if u_mode == 'linspace' else (u[1] if u_mode == 'shared' else u).cuda().contiguous()
                bd, wd = bins.cuda().contiguous(), w.cuda().contiguous()
                smp, cdf, inds = out(n, N), out(n, n_bins), torch.full((n, N), -7, dtype=torch.int32, device='cuda')
                check(L.nerf_sample_pdf_ex(p(bd), p(wd), n, n_bins, p(u), int(u_mode == 'per ray'), N, p(smp), p(cdf), p(inds), current_stream()))
                print(f'sample_pdf n_bins={n_bins} N={N} u={u_mode}: {sha([smp, cdf, inds])}', flush=True)

    # ---- merge and sort: the cases of tests/test_scan_special_gpu.py
    for na, nb in MERGE_SHAPES + [(1, 1)]:
        a, b = merge_case(na, nb)[:2]
        ad, bd, o = a.cuda().contiguous(), b.cuda().contiguous(), out(MERGE_ROWS, na + nb)
        check(L.nerf_merge_sorted(p(ad), na, p(bd), nb, MERGE_ROWS, p(o), current_stream()))
        print(f'merge {na}+{nb}: {sha([o])}', flush=True)
    for N in SORT_N:
        x = sort_case(N)[0].cuda().contiguous()
        o = out(x.shape[0], N)
        check(L.nerf_sort_rows(p(x), x.shape[0], N, p(o), current_stream()))
        print(f'sort {N}: {sha([o])}', flush=True)

    # ---- the engine: the fused coarse scan and its three launches
    H = 21
    sds = (O.make_teacher_state(1), O.make_teacher_state(2))
    for S0, NI in ENGINE:
        for white in (False, True):
            eng = NeRFEngine(H, H, O.focal_from_angle(H), N_samples=S0, N_importance=NI, white_bkgd=white).load_state_dicts(*sds)
            ro, rd = O.get_rays(H, H, eng.focal, O.pose_spherical(12., -33., 4.)[:3, :4])
            ro, rd = ro.reshape(-1, 3)[:H * H - 3].float().clone(), rd.reshape(-1, 3)[:H * H - 3].float().clone()
            for ray in range(0, ro.shape[0], 4):
                poison_ray(ro, rd, ray, (ray // 4) % len(RAY_POISONS))
            ro, rd = ro.cuda().contiguous(), rd.cuda().contiguous()
            for noise in (0., 0.7):
                for split in (0, 1):
                    check(L.nerf_debug_set_split_scans(eng._ctx, split))
                    got = eng.render_rays(ro, rd, extras=True, raw_noise_std=noise, pytest=True)
                    print(f'engine {S0}+{NI} white={int(white)} noise={noise} split={split}: {sha(got[k] for k in sorted(got))}', flush=True)
            eng.close()


if __name__ == '__main__':
    main()

"""CPU: FLIP's host side (efficient-nerf_amd/flip_taps.py, the argument checks of r2l_flip, the --test_flip flag).

The reference's dense 2-D filters in tests/golden/flip.npz (make_golden_flip.py: utils/flip_loss.py's own, float32, at
pixels_per_degree 67.02 and 30) are reassembled from the 1-D taps the kernels filter with."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAP_ROWS = ('A', 'RG', 'BY1', 'BY2', 'G', 'D', 'P')            # r2l_flip_taps' rows


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'flip.npz'))


def _reassembled(FT, ppd):
    c, f = FT.csf_taps(ppd, np.float64), FT.feature_taps(ppd, np.float64)
    return {'A': np.outer(c['A'], c['A']), 'RG': np.outer(c['RG'], c['RG']),
            'BY': np.outer(c['BY1'], c['BY1']) + np.outer(c['BY2'], c['BY2']),          # the two-term sum
            'edge': np.outer(f['G'], f['D']), 'point': np.outer(f['G'], f['P'])}        # [y, x]: the first factor runs along x


def test_taps_reassemble_the_reference_filters(pkg, golden):
    """float64 outer products of the 1-D taps against the stored float32 filters: within 2 float32 ulps of the largest tap (the
    stored filter is rounded once, half an ulp of each of its own taps; the point filter's two normalisations are float32
    divisions in the reference, another half)"""
    from efficient_nerf_amd import flip_taps as FT
    for j, ppd in enumerate(golden['ppds']):
        for name, mine in _reassembled(FT, float(ppd)).items():
            ref = golden[f'dense_{name}_{j}']
            assert ref.dtype == np.float32 and ref.shape == mine.shape
            gap, ulp = np.abs(ref.astype(np.float64) - mine).max(), np.abs(ref).max() * 2.0 ** -23
            print(f'pixels_per_degree {ppd:.2f} {name}: {ref.shape[0]} x {ref.shape[1]}, worst gap {gap:.3e} = {gap / ulp:.2f} ulp of the largest tap')
            assert gap <= 2 * ulp
        # the signs of the point filter are normalised apart: positive weights sum to 1, negative ones to -1
        f = FT.feature_taps(float(ppd), np.float64)
        for t in (np.outer(f['G'], f['D']), np.outer(f['G'], f['P'])):
            assert abs(t[t > 0].sum() - 1) < 1e-12 and abs(t[t < 0].sum() + 1) < 1e-12


def test_radii_are_the_reference_s(pkg, golden):
    from efficient_nerf_amd import flip_taps as FT
    assert abs(FT.FLIP_PPD - float(golden['ppds'][0])) < 1e-12
    for j, ppd in enumerate(golden['ppds']):
        r_c, r_f = FT.radii(float(ppd))
        assert golden[f'dense_A_{j}'].shape == golden[f'dense_BY_{j}'].shape == (2 * r_c + 1,) * 2
        assert golden[f'dense_edge_{j}'].shape == golden[f'dense_point_{j}'].shape == (2 * r_f + 1,) * 2
    assert FT.radii(FT.FLIP_PPD) == (10, 9) and FT.radii(30.) == (5, 4)


def test_library_taps_are_the_numpy_taps(pkg, built_lib, golden):
    """r2l_flip_taps (what the kernels get) against flip_taps.py: the same float64 formulas in C and in numpy, so at most the
    last float32 bit apart (the two exp() need not round alike)"""
    from efficient_nerf_amd import _lib, flip_taps as FT
    L = _lib.lib()
    for ppd in list(golden['ppds']) + [FT.MAX_RADIUS / (3 * np.sqrt(0.04 / (2 * np.pi ** 2))) - 1e-6]:
        buf, rc, rf = (C.c_float * (7 * 33))(), C.c_int(), C.c_int()
        assert L.r2l_flip_taps(float(ppd), buf, C.byref(rc), C.byref(rf)) == 0
        assert (rc.value, rf.value) == FT.radii(float(ppd))
        got = np.array(buf, dtype=np.float32).reshape(7, 33)
        want = dict(FT.csf_taps(float(ppd)), **FT.feature_taps(float(ppd)))
        for k, name in enumerate(TAP_ROWS):
            n = 2 * (rc.value if k < 4 else rf.value) + 1
            assert np.all(got[k, n:] == 0)
            assert np.all(np.abs(got[k, :n] - want[name]) <= np.spacing(np.abs(want[name]))), name
    assert FT.radii(float(ppd))[0] == FT.MAX_RADIUS


def test_flip_checks_its_arguments(pkg, built_lib):
    """R2L_EINVAL with a message on NULL or bad arguments, before any device is looked for"""
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.r2l_last_error().decode()
    p, q, ws = C.c_void_p(0x1000), C.c_void_p(0x100000), C.c_void_p(0x200000)
    ppd = 67.02
    need = L.r2l_flip_workspace_floats(8, 8, ppd)
    assert need >= 14 * 64
    ident = (0., 1., 0.) * 2
    f = L.r2l_flip
    assert f(None, p, 1, 8, 8, *ident, ppd, None, q, ws, need, None) == -1 and 'r2l_flip' in err() and 'NULL' in err()
    assert f(p, None, 1, 8, 8, *ident, ppd, None, q, ws, need, None) == -1 and 'NULL' in err()
    assert f(p, p, 1, 8, 8, *ident, ppd, None, None, ws, need, None) == -1 and 'NULL' in err()
    assert f(p, p, 1, 0, 8, *ident, ppd, None, q, ws, need, None) == -1 and 'H=0' in err()
    assert f(p, p, 1, 8, 0, *ident, ppd, None, q, ws, need, None) == -1 and 'W=0' in err()
    assert f(p, p, -1, 8, 8, *ident, ppd, None, q, ws, need, None) == -1 and 'n_img=-1' in err()
    assert f(p, p, 1, 8, 8, *ident, 200., None, q, ws, need, None) == -1 and 'radius of 28' in err() and 'up to 16' in err() and '118.47' in err()
    for bad in (0., -3., float('nan')):
        assert f(p, p, 1, 8, 8, *ident, bad, None, q, ws, need, None) == -1 and 'pixels_per_degree' in err()
    assert f(p, p, 1, 8, 8, *ident, ppd, None, q, ws, need - 1, None) == -1 and f'needs {need}' in err()
    assert f(p, p, 1, 8, 8, *ident, ppd, None, q, C.c_void_p(0x200002), need, None) == -1 and 'aligned' in err()
    assert L.r2l_flip_workspace_floats(0, 8, ppd) == -1 and L.r2l_flip_workspace_floats(8, 8, 200.) == -1 and 'radius' in err()
    assert f(None, None, 0, 8, 8, *ident, ppd, None, None, None, 0, None) == 0          # n_img = 0: a no-op, whatever the pointers
    assert f(None, None, 0, 8, 8, *ident, 200., None, None, None, 0, None) == -1        # ... but not whatever the arguments


def test_flag_parses_and_defaults_to_off(pkg):
    from efficient_nerf_amd.frontend import parse_args
    base = ['--model_name', 'R2L', '--render_only', '--pretrained_ckpt', 'x.tar']
    assert parse_args(base).test_flip is False
    assert parse_args(base + ['--test_flip']).test_flip is True


def test_flip_refuses_what_the_kernels_do_not_take(pkg):
    import torch
    from efficient_nerf_amd import metrics
    with pytest.raises(ValueError, match='one shape'):
        metrics.flip(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 5, 3))
    with pytest.raises(ValueError, match='GPU'):
        metrics.flip(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 3))

"""The 1-D taps of FLIP's five filters (utils/flip_loss.py:137-181, 259-288), pure numpy: the host mirror of what
csrc/r2l_flip.hip builds for its kernels (r2l_flip_taps returns the library's own; tests/test_flip_cpu.py compares the two and
reassembles the reference's dense 2-D filters from them).

Every one of the reference's filters is separable or a sum of two separable ones:
  A, RG   a1 sqrt(pi/b1) exp(-pi^2 (x^2 + y^2) dx^2 / b1) / sum (their a2 is 0)    = n (x) n,  n = e / sum(e)
  BY      (w1 E1 + w2 E2) / S,  Ei = ei (x) ei,  S = w1 sum(e1)^2 + w2 sum(e2)^2   = t1 (x) t1 + t2 (x) t2,  ti = sqrt(wi / S) ei
  edge    -x g(x) g(y), positive and negative weights normalised apart             = d (x) gn
  point   (x^2 / sd^2 - 1) g(x) g(y), likewise; the sign depends on x alone        = p (x) gn
All in float64, rounded to float32 once at the end."""
import math

import numpy as np

FLIP_PPD = 0.7 * (3840 / 0.7) * (np.pi / 180)         # main.py:373-377: 0.7 m from a 0.7 m wide 3840-pixel monitor, 67.02
MAX_RADIUS = 16                                        # what the kernels' tiles hold (csrc/r2l_flip.hip FLIP_MAX_R)
_CSF = {'A': (1, 0.0047, 0, 1e-5), 'RG': (1, 0.0053, 0, 1e-5), 'BY': (34.1, 0.04, 13.5, 0.025)}
_W_EDGE = 0.082


def radii(pixels_per_degree):
    """(CSF radius, feature radius) as the reference derives them (:167-170, :267-268)"""
    r_c = int(np.ceil(3 * np.sqrt(0.04 / (2 * np.pi ** 2)) * pixels_per_degree))
    r_f = int(np.ceil(3 * (0.5 * _W_EDGE * pixels_per_degree)))
    return r_c, r_f


def csf_taps(pixels_per_degree, dtype=np.float32):
    """{'A': n, 'RG': n, 'BY1': t1, 'BY2': t2}, each [2 r_c + 1]: A = n (x) n, RG likewise, BY = t1 (x) t1 + t2 (x) t2"""
    r, _ = radii(pixels_per_degree)
    x2 = (np.arange(-r, r + 1, dtype=np.float64) / pixels_per_degree) ** 2
    out = {}
    for name, (a1, b1, a2, b2) in _CSF.items():
        e1, e2 = np.exp(-np.pi ** 2 * x2 / b1), np.exp(-np.pi ** 2 * x2 / b2)
        w1, w2 = a1 * math.sqrt(np.pi / b1), a2 * math.sqrt(np.pi / b2)
        if name == 'BY':
            s = w1 * e1.sum() ** 2 + w2 * e2.sum() ** 2
            out['BY1'], out['BY2'] = math.sqrt(w1 / s) * e1, math.sqrt(w2 / s) * e2
        else:                       # a2 = 0: one Gaussian
            out[name] = e1 / e1.sum()
    return {k: v.astype(dtype) for k, v in out.items()}


def feature_taps(pixels_per_degree, dtype=np.float32):
    """{'G': gn, 'D': d, 'P': p}, each [2 r_f + 1]: the edge filter along x is d (x) gn, the point filter p (x) gn (first factor
    along x), and their transposes along y"""
    _, r = radii(pixels_per_degree)
    sd = 0.5 * _W_EDGE * pixels_per_degree
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-x ** 2 / (2 * sd * sd))
    d, p = -x * g, (x ** 2 / (sd * sd) - 1) * g
    out = {'G': g / g.sum()}
    for name, t in (('D', d), ('P', p)):
        pos, neg = t[t > 0].sum(), -t[t < 0].sum()
        out[name] = np.where(t < 0, t / neg, t / pos)
    return {k: v.astype(dtype) for k, v in out.items()}

"""Golden vectors for FLIP at the edges of the kernels' tiles and filter radii (csrc/r2l_flip.hip; tests/test_flip_gpu.py): the
REFERENCE's own utils/flip_loss.py, unmodified, imported through make_golden_flip.py (its stand-ins for .cuda() and its float32 /
float64 runner), at generation time only (build container only):

    python tests/golden/make_golden_flip_edges.py

CASES are natural pairs, pair(g, h, w, 0.03), at three viewing geometries: pixels_per_degree 118 gives the filter radii (16, 15), the
largest the kernels hold; 5 gives (1, 1), the smallest there are; 16 gives (3, 2).  The shapes are strips one pixel wide, a frame
smaller than every filter, exact multiples of the column kernel's 64 x 32 tile and of the row kernel's 128 pixels, and one pixel past
them.  The last case is a 48 x 56 pair at the default geometry (radii 10 and 9) with a[20, 30, 1] = NaN and b[5, 5, 0] = +Inf: the
reference's dense 21 x 21 filters turn the NaN into the box of rows 10 .. 30 and columns 20 .. 40 and nothing else (asserted here, in
both precisions); the Inf is clamped to 1 by the sRGB transform and stays finite.

flip_edges.npz has flip.npz's per-case layout: a_k, b_k [H, W, 3] (float16-exact values, stored as float16), ppd_k, map64_k [H, W] and
mean64_k (compute_flip in float64), band_k = L_inf(float32 map - float64 map), over the finite pixels of the float64 map in the last
case."""
import os

import numpy as np
import torch

import make_golden_flip as G      # the reference's flip_loss.py on the CPU, pair() and run()

torch.set_num_threads(1)          # the same sums in the same order wherever this runs
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((118.0, ((1, 70), (70, 1), (3, 5), (32, 64), (32, 128), (33, 129))),
         (5.0, ((3, 5), (1, 70), (33, 129))),
         (16.0, ((70, 1), (32, 64))))
NAN_AT, INF_AT, NAN_BOX = (20, 30, 1), (5, 5, 0), (slice(10, 31), slice(20, 41))


if __name__ == '__main__':
    g = torch.Generator().manual_seed(29)
    cases = [G.pair(g, h, w, 0.03) + (ppd,) for ppd, shapes in CASES for h, w in shapes]
    a, b = (t.half().float() for t in G.pair(g, 48, 56, 0.03))
    a[NAN_AT], b[INF_AT] = float('nan'), float('inf')
    cases.append((a, b, G.PPD))
    out = {}
    for k, (a, b, ppd) in enumerate(cases):
        a, b = a.half().float(), b.half().float()
        m64 = G.run(a, b, ppd, False, torch.float64)
        m32 = G.run(a, b, ppd, False, torch.float32)
        assert m64.dtype == np.float64 and m32.dtype == np.float32 and m64.shape == tuple(a.shape[:2])
        finite = np.isfinite(m64)
        if k == len(cases) - 1:
            box = np.zeros(m64.shape, dtype=bool)
            box[NAN_BOX] = True
            assert np.array_equal(np.isnan(m64), box) and np.array_equal(np.isnan(m32), box) and box.sum() == 21 * 21
            assert np.array_equal(finite, ~box)
        else:
            assert finite.all() and np.isfinite(m32).all()
        out[f'a_{k}'], out[f'b_{k}'] = a.numpy().astype(np.float16), b.numpy().astype(np.float16)
        out[f'ppd_{k}'] = np.float64(ppd)
        out[f'map64_{k}'], out[f'mean64_{k}'] = m64, np.float64(m64.mean())
        out[f'band_{k}'] = np.float64(np.abs(m32.astype(np.float64) - m64)[finite].max())
        print(k, tuple(a.shape[:2]), f'ppd {ppd:.2f}: mean {m64.mean():.6f} band {out[f"band_{k}"]:.2e}, {int((~finite).sum())} NaN pixels')
    path = os.path.join(HERE, 'flip_edges.npz')
    np.savez_compressed(path, **out)
    print('flip_edges.npz', len(out), 'arrays', os.path.getsize(path), 'bytes')

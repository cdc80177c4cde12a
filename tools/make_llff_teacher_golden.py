"""Golden rows for the LLFF teacher's ray batches: what the REFERENCE's use_batching bank holds for 256 fixed rows of the fixture
scene, and what its render() makes of them.

    python tools/make_llff_teacher_golden.py PATH_TO_REFERENCE

Runs the reference's own utils/run_nerf_raybased_helpers.py (get_rays_np, ndc_rays) on the CPU and restates nothing but the glue of
main.py:1141-1154 (the bank: get_rays_np of every pose beside the images, training views only, [n, 3, 3] float32) and of
main.py:148-162 (viewdirs = rays_d / ||rays_d|| of the world rays, then ndc_rays(H, W, focal, 1., ...)).  The scene comes through
efficient-nerf_amd/llff.py, whose images, poses and bounds equal the reference loader's (tests/test_llff_cpu.py).  Writes
tests/golden/llff_teacher/rows.npz: data only.  No test imports the reference; the tests read the file."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(reference):
    sys.path.insert(0, reference)
    import utils.run_nerf_raybased_helpers as RH          # the reference's
    import _pkg
    _pkg.load()
    from efficient_nerf_amd import llff
    scene = llff.load_scene(os.path.join(ROOT, 'tests', 'golden', 'llff', 'scene'), 8)
    images, poses = scene.images, scene.poses
    hwf = poses[0, :3, -1]
    # main.py:988 makes focal a Python float, which get_rays_np's to_array() does not take (it reads .data of anything that is not an
    # ndarray).  A Python float leaves the float32 pixel grid in float32; a 0-d float32 array of the same value does the same under
    # every numpy (a float64 array would lift the arithmetic to float64 under numpy 2)
    H, W, focal = int(hwf[0]), int(hwf[1]), np.array(float(hwf[2]), dtype=np.float32)
    assert float(focal) == float(hwf[2])
    poses = poses[:, :3, :4]
    i_test = np.arange(images.shape[0])[::8]
    i_train = np.array([i for i in np.arange(int(images.shape[0])) if i not in i_test])
    rays = np.stack([RH.get_rays_np(H, W, focal, p) for p in poses[:, :3, :4]], 0)       # main.py:1141-1154
    rays_rgb = np.concatenate([rays, images[:, None]], 1)
    rays_rgb = np.transpose(rays_rgb, [0, 2, 3, 1, 4])
    rays_rgb = np.stack([rays_rgb[i] for i in i_train], 0)
    rays_rgb = np.reshape(rays_rgb, [-1, 3, 3]).astype(np.float32)
    n = rays_rgb.shape[0]
    rows = np.sort(np.random.RandomState(20).choice(n, 256, replace=False)).astype(np.int64)
    rows[0], rows[-1] = 0, n - 1
    batch = torch.from_numpy(rays_rgb[rows])
    rays_o, rays_d, target = batch[:, 0], batch[:, 1], batch[:, 2]
    viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)                          # main.py:154-157
    ndc_o, ndc_d = RH.ndc_rays(H, W, float(focal), 1., rays_o, rays_d)                    # main.py:162
    out = os.path.join(ROOT, 'tests', 'golden', 'llff_teacher')
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, 'rows.npz'), rows=rows, n=np.int64(n), H=np.int64(H), W=np.int64(W), focal=np.float64(focal),
             rays_o=rays_o.numpy(), rays_d=rays_d.numpy(), target=target.numpy(), viewdirs=viewdirs.float().numpy(),
             ndc_o=ndc_o.float().numpy(), ndc_d=ndc_d.float().numpy())
    print(f'{n} bank rows of {len(i_train)} training views {H} x {W}, focal {float(focal):.6f}; wrote 256 rows to {out}/rows.npz')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])

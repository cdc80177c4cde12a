"""What the non-finite-ray pass costs: the three entry points of the R2L student at 800 x 800 (W256D88, fp16_fp8) and
one NeRF-teacher frame at 400 x 400 (64 + 128 samples, fp16x1), each as HIP-event windows after a warm-up: median [min .. max] per call.

  render        host pose: twelve comparisons on the host, no extra launch for a finite pose (what bench.py renders through)
  render_batch  one device pose: r2l_mark_nonfinite_kernel behind the tail
  render_rays   640,000 given rays: the same kernel, which reads the rays (24 B each) once more
  teacher       nerf_mark_nonfinite_kernel behind both MLP launches (24 B + two depths per ray and launch)

To compare two builds, run it once per build in a process of its own, alternating (R2L_LIB_PATH selects the library, efficient-nerf_amd/_lib.py):
  R2L_LIB_PATH=/path/to/before.so python tools/nonfinite_time.py; python tools/nonfinite_time.py; ... (profiles/nonfinite_time.txt)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import NeRFEngine, PRECISIONS, R2LEngine, get_rays  # noqa: E402
from oracle import r2l_oracle as O  # noqa: E402


def windows(fn, calls, n_windows, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def line(name, ms):
    print(f'  {name}: {statistics.median(ms):.4f} ms [{min(ms):.4f} .. {max(ms):.4f}]', flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    a = ap.parse_args()
    from efficient_nerf_amd import _lib
    print(f'library: {os.path.basename(_lib.LIB_PATH)}', flush=True)
    H = 800
    focal = O.focal_from_angle(H)
    eng = R2LEngine(H, H, focal, n_block=43, precision=PRECISIONS['fp16_fp8']).load_state_dict(O.make_r2l_state(0))
    c2w = torch.as_tensor(O.pose_spherical(30., -30., 4.))[:3, :4].float().contiguous()
    dev_pose = c2w.cuda().reshape(1, 3, 4)
    ro, rd = get_rays(H, H, focal, c2w, device='cuda')
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    out = torch.empty((H * H, 3), device='cuda')
    line('R2L 800 x 800 fp16_fp8, render (host pose)', windows(lambda: eng.render(c2w, out=out), a.calls, a.windows, 5))
    line('R2L 800 x 800 fp16_fp8, render_batch (one device pose)', windows(lambda: eng.render_batch(dev_pose, out=out[None]), a.calls, a.windows, 5))
    line('R2L 800 x 800 fp16_fp8, render_rays (640,000 given rays)', windows(lambda: eng.render_rays(ro, rd, out=out), a.calls, a.windows, 5))
    eng.close()
    Ht = 400
    teng = NeRFEngine(Ht, Ht, O.focal_from_angle(Ht), precision=PRECISIONS['fp16x1']).load_state_dicts(O.make_teacher_state(1), O.make_teacher_state(2))
    line('teacher 400 x 400, 64 + 128 samples, fp16x1, render', windows(lambda: teng.render(c2w), 3, a.windows, 2))
    teng.close()


if __name__ == '__main__':
    main()

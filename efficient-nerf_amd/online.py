"""Online distillation: the teacher renders every step's rays on the card the student trains on.

The reference's pipeline meets on the disk: `create_data rand` writes the teacher's renders of 10,000 random poses as ray shards and
`main.py` reads 20 of them per step, because its teacher takes seconds per frame.  Here the teacher (NeRFEngine) and the student's
trainer (train.R2LTrainer) are launches of one library on one device, so a step can ask for fresh rays instead:

    OnlineTeacherSource.batch(step, n)
        host     n_pose random poses and focals, the draws of create_data rand in its order (per pose theta, phi, then the focal
                 scale: RandStream.rand_pose / rand_focal_scale) from np.random.RandomState((seed, step))
        device   one r2l_rand_rays launch (csrc/r2l_online.hip): ray k = a Philox-drawn pixel of pose k % n_pose, get_rays' ray
        device   engine.render_rays(rays_o, rays_d)['rgb_map']: the target

On a mounted LLFF scene (LLFFOnlineTeacherSource) the poses are the reference's get_rand_pose_v2 in the scene's pose boxes, and they are
built on the device too: the host draws the step's n_pose x 7 uniforms in LLFFRandStream's order (one RandomState.rand call) and uploads
them, r2l_llff_rand_poses makes poses and focals from them, and r2l_rand_rays and the NDC teacher (at the base focal, as create_data
rand projects) follow as above -- two launches a step, and no pose exists on the host.

A batch is a function of (seed, step) alone -- nothing of the source has to be saved in a checkpoint, and a resumed run sees the
batches the uninterrupted run saw.  (The teacher's mode is the one exception: `--precision auto` measures it again at start-up, and a
watch that stepped down in the first run has to step down again; the modes differ by less than the watch's limits.)

The watch of create_rand and render_path carries over: every watch_every-th step the batch is spot-checked against fp16x3 before it
is handed on (NeRFEngine.spot_check); a miss moves the engine one rung down its ladder and the batch is rendered again."""
import os

import numpy as np
import torch

from ._lib import R2LError, check, current_stream, dptr, lib


class OnlineTeacherSource:
    """engine: what renders the targets (render_rays(rays_o, rays_d) -> {'rgb_map': [n, 3]}; spot_check / step_down / set_skip_rgb0
    where it has them: NeRFEngine, or generic.GenericNeRF for teachers outside the fused kernels).  (H, W, focal): the camera the
    random poses look through; with use_rand_focal every pose draws its own focal in [focal, 2 focal).  watch_every: 0 = never.
    rays_fn(poses [n_pose, 3, 4], focals [n_pose] float32, step, n) -> (rays_o, rays_d): replaces the r2l_rand_rays launch."""

    def __init__(self, engine, H, W, focal, n_pose=100, seed=0, use_rand_focal=True, watch_every=100, log=print, rays_fn=None):
        self.engine, self.H, self.W, self.focal = engine, int(H), int(W), float(focal)
        self.n_pose, self.seed, self.use_rand_focal = int(n_pose), int(seed), bool(use_rand_focal)
        self.watch_every, self.log = int(watch_every), log or (lambda *a, **k: None)
        if self.n_pose < 1 or not 1 <= self.H * self.W < 2 ** 31 or not self.focal > 0:
            raise R2LError(f'n_pose={n_pose} H={H} W={W} focal={focal}')
        if not 0 <= self.seed < 2 ** 32 or self.watch_every < 0:
            raise R2LError(f'seed={seed} (0 .. 2^32 - 1: one word of the RandomState seed) watch_every={watch_every}')
        self.device = torch.device(getattr(engine, 'device', 'cpu'))
        self._rays_fn = rays_fn or self._launch_rays
        from .watch import Watch
        self._watch = Watch(len(getattr(engine, 'LADDER', (0,))), log=self.log)
        if hasattr(engine, 'set_skip_rgb0'):
            engine.set_skip_rgb0(True)        # only rgb_map is taken (as create_rand does): the coarse pass runs without its view branch

    checks = property(lambda self: self._watch.checks)           # the watch's two counters
    fallbacks = property(lambda self: self._watch.fallbacks)

    def draws(self, step):
        """(poses [n_pose, 3, 4] float32, focals [n_pose] float64) of a step, on the host"""
        from .create_data import RandStream
        if not 0 <= int(step) < 2 ** 32:
            raise R2LError(f'step={step}')
        stream = RandStream(seed=(self.seed, int(step)), n_loader_poses=0)
        poses, focals = [], np.empty(self.n_pose, dtype=np.float64)
        for p in range(self.n_pose):
            poses.append(stream.rand_pose()[:3, :4])
            focals[p] = self.focal * stream.rand_focal_scale() if self.use_rand_focal else self.focal
        return torch.stack(poses, 0).contiguous(), focals

    def poses(self, step):
        """(poses [n_pose, 3, 4], focals [n_pose]) of a step as float32 tensors, as rays_fn takes them: on the host here (the ray
        launch uploads them); get_rays rounds the focal the same way"""
        poses, focals = self.draws(step)
        return poses, torch.from_numpy(focals).to(torch.float32)

    def _launch_rays(self, poses, focals, step, n):
        dev = self.device
        po, fo = poses.to(dev), focals.to(dev)
        ro = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rd = torch.empty((n, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib().r2l_rand_rays(dptr(po), dptr(fo), self.n_pose, self.H, self.W, self.seed, int(step), n, dptr(ro), dptr(rd), None,
                                      current_stream()))
        return ro, rd

    def batch(self, step, n, rows=None, group=None):
        """(rays_o, rays_d, target), each [n, 3] float32 on the engine's device.  rows = (r0, r1) on a rank of a ray-sharded run
        (torch.distributed group `group`): every rank draws the poses and launches the rays of all n, renders the targets of its
        rows only, and the targets are all-gathered (the hard-ray pool needs every row); on a watched step a rank checks its own
        rows, a miss on any rank (one MAX all-reduce) moves every rank's engine one rung down, and all render again."""
        step, n = int(step), int(n)
        ro, rd = self._rays_fn(*self.poses(step), step, n)
        eng = self.engine
        if rows is None:
            lro, lrd, any_rank = ro, rd, bool
        else:
            from . import dist as D
            r0, r1 = rows
            lro, lrd = ro[r0:r1].contiguous(), rd[r0:r1].contiguous()
            any_rank = lambda flag: D.any_rank(flag, self.device, group)

        def render():
            if lro.shape[0] == 0:
                return {'rgb_map': torch.empty((0, 3), dtype=torch.float32, device=ro.device)}
            return eng.render_rays(lro, lrd)

        def step_down(ok, d):
            was = getattr(eng, 'precision_name', '?')
            now = eng.step_down()
            what = d if not ok else 'off on the rows of another rank,'
            line = (f'[precision] step {step}: {was} is {what} from fp16x3 on {getattr(eng, "WATCH_RAYS", "a sample")} of the batch\'s rays '
                    f'-> {now}; batch rendered again')
            return {'step': step, 'from': was, 'to': now, 'diffs': d}, line if rows is None or D.rank_world(group)[0] == 0 else None   # one line per run, not per rank

        out = render()
        if self.watch_every and step % self.watch_every == 0 and hasattr(eng, 'spot_check'):
            # a rank without rows has nothing to compare, but it enters every collective and counts the check
            out = self._watch.run(out, check=lambda got: eng.spot_check(lro, lrd, got) if lro.shape[0] else (True, {}), step_down=step_down,
                                  again=render, agree=any_rank)
        target = out['rgb_map']
        if rows is not None:
            import torch.distributed as td
            target = D.gather_rows(target[None].contiguous(), n, 1, td.get_world_size(group), group)[0]
        return ro, rd, target


class LLFFOnlineTeacherSource(OnlineTeacherSource):
    """The same source on an LLFF scene: a step's poses are llff.pose_in_boxes' (the reference's get_rand_pose_v2) in the pose boxes
    of `state` (the loaded scene's llff.RandPoseState), built on the device by r2l_llff_rand_poses from the step's uniform draws --
    per pose the six draws of LLFFRandStream.rand_pose and then the focal scale, in that order -- so the host's part of a step is one
    RandomState.rand call and its upload, and no pose exists on the host.  engine: the NDC teacher (near, far = 0, 1) at the base
    focal, create_data.build_llff_teacher_engine's."""

    def __init__(self, engine, H, W, focal, state, **kw):
        from . import llff
        super().__init__(engine, H, W, focal, **kw)
        self.box = np.ascontiguousarray(llff.pose_box(state), dtype=np.float64)
        self.n_u = 7 if self.use_rand_focal else 6

    def uniforms(self, step):
        """the step's draws, float64 [n_pose, n_u]: row k is pose k's position (x, y, z), viewing axis (x, y, z) and focal scale - 1"""
        if not 0 <= int(step) < 2 ** 32:
            raise R2LError(f'step={step}')
        return np.random.RandomState((self.seed, int(step))).rand(self.n_pose, self.n_u)

    def poses(self, step):
        """(poses [n_pose, 3, 4], focals [n_pose]) float32 on the device: one upload and one launch"""
        import ctypes as C
        dev = self.device
        u = torch.from_numpy(self.uniforms(step)).to(dev)
        po = torch.empty((self.n_pose, 3, 4), dtype=torch.float32, device=dev)
        fo = torch.empty((self.n_pose,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib().r2l_llff_rand_poses(C.c_void_p(u.data_ptr()), self.n_pose, self.n_u, self.box.ctypes.data_as(C.c_void_p), self.focal,
                                            dptr(po), dptr(fo), current_stream()))
        return po, fo

    def draws(self, step):
        """the kernel's poses and focals of a step read back: (poses [n_pose, 3, 4] float32, focals [n_pose] float64) on the host"""
        po, fo = self.poses(step)
        return po.cpu(), fo.cpu().numpy().astype(np.float64)


def agree_teacher_precision(eng, group=None):
    """`--precision auto` measures the teacher's mode at start-up on every rank; the ranks render rows of the same batches, so rank 0's
    (fine, coarse) pair is broadcast and adopted.  No-op for one rank and for engines without modes (the generic fp32 path)."""
    import torch.distributed as td
    if not td.is_initialized() or td.get_world_size(group) == 1 or not hasattr(eng, 'set_precision_pair'):
        return
    obj = [(int(eng.precision), int(eng.precision_coarse))]
    td.broadcast_object_list(obj, src=td.get_global_rank(group, 0) if group is not None else 0, group=group)
    if obj[0] != (int(eng.precision), int(eng.precision_coarse)):
        eng.set_precision_pair(obj[0][1], obj[0][0])


def check_online_args(args):
    """the command lines --kd_online refuses, one line each"""
    from . import frontend as fe
    if args.datadir_kd:
        raise SystemExit(f'--kd_online renders every step\'s rays with the teacher; --datadir_kd {args.datadir_kd} names ray shards: pass one of the two')
    if not args.teacher_ckpt:
        raise SystemExit('--kd_online needs --teacher_ckpt X.tar (the NeRF teacher that renders the rays)')
    if fe.has_llff_scene(args):            # the poses come from the scene's own pose boxes (LLFFOnlineTeacherSource)
        if args.no_ndc:
            raise SystemExit('--kd_online on --dataset_type llff renders the NDC teacher: --no_ndc is not built here')
    elif args.dataset_type != 'blender':
        why = ''
        if args.dataset_type == 'llff':
            why = ('; on an LLFF scene they are drawn in the scene\'s pose boxes, but ' +
                   ('--synthetic_poses is set' if args.synthetic_poses > 0 else f'"{os.path.join(args.datadir, "poses_bounds.npy")}" is not there'))
        raise SystemExit(f'--kd_online with --dataset_type {args.dataset_type}: the random poses are Blender\'s hemisphere (--dataset_type blender)' + why)
    if args.kd_online_poses < 1 or args.kd_online_split < 1 or args.kd_online_watch < 0 or not 0 <= args.kd_online_seed < 2 ** 32:
        raise SystemExit(f'--kd_online_poses {args.kd_online_poses} --kd_online_split {args.kd_online_split} --kd_online_watch '
                         f'{args.kd_online_watch} --kd_online_seed {args.kd_online_seed}: at least one pose and one ray, a watch interval >= 0, a seed '
                         f'in 0 .. 2^32 - 1')


def teacher_args(args):
    """The teacher's own flags (use_viewdirs, N_samples, N_importance, white_bkgd, half_res, the network's shape): --teacher_config, by
    default configs' lego.txt beside the student's --config; on a mounted LLFF scene <the scene's folder name>.txt there (fern.txt
    for .../nerf_llff_data/fern).  The scene, the image size (LLFF: --factor, --llffhold, --spherify) and --precision are the command
    line's."""
    from . import frontend as fe
    llff = fe.has_llff_scene(args)
    default = os.path.basename(os.path.normpath(args.datadir)) + '.txt' if llff else 'lego.txt'
    path = args.teacher_config or (os.path.join(os.path.dirname(os.path.abspath(args.config)), default) if args.config else '')
    if not path or not os.path.exists(path):
        raise SystemExit(f'--kd_online reads the teacher\'s flags from --teacher_config FILE (default: {default} beside --config): '
                         f'"{path}" is not there')
    t = fe.parse_args(['--config', path])
    t.datadir, t.H, t.W, t.synthetic_poses, t.precision = args.datadir, args.H, args.W, args.synthetic_poses, args.precision
    if llff:
        t.dataset_type, t.factor, t.llffhold, t.spherify = 'llff', args.factor, args.llffhold, args.spherify
    return t


def source_from_args(args, log=print):
    """(OnlineTeacherSource, the start-up line's description of it) for train.train under --kd_online, which has refused what
    check_online_args refuses"""
    from . import frontend as fe
    from .create_data import build_llff_teacher_engine, build_teacher_engine
    t = teacher_args(args)
    ckpt = fe.load_checkpoint(args.teacher_ckpt)
    rand_focal = not args.no_rand_focal
    watched = f'every {args.kd_online_watch} steps' if args.kd_online_watch else 'never (--kd_online_watch 0)'
    kw = dict(n_pose=args.kd_online_poses, seed=args.kd_online_seed, use_rand_focal=rand_focal, watch_every=args.kd_online_watch, log=log)
    if fe.has_llff_scene(args):
        from . import llff
        if t.no_ndc:
            raise SystemExit('--kd_online on --dataset_type llff renders the NDC teacher: the teacher\'s flags ask for no_ndc, which is not built here')
        try:
            scene = llff.load_scene(args.datadir, args.factor, spherify=args.spherify, decode=fe.png_reader(args))
        except llff.LLFFError as e:           # the loader's refusals are one line each
            raise SystemExit(str(e))
        H, W, focal = scene.hwf
        eng = build_llff_teacher_engine(t, ckpt, (H, W, focal), scene.rand_state, rand_focal, log=log, watched=watched)
        src = LLFFOnlineTeacherSource(eng, H, W, focal, scene.rand_state, **kw)
        where = f' (drawn on the device in the pose boxes of "{args.datadir}", NDC teacher at the base focal)'
    else:
        _, (H, W, focal) = fe.load_test_poses(t)
        eng = build_teacher_engine(t, ckpt, (H, W, focal), rand_focal, log=log, watched=watched)
        src = OnlineTeacherSource(eng, H, W, focal, **kw)
        where = ''
    mode = getattr(eng, 'precision_name', 'fp32')
    what = (f'teacher "{args.teacher_ckpt}" in {mode}' + (' (chosen by --precision auto)' if args.precision == 'auto' and mode != 'fp32' else '') +
            f', {src.n_pose} random poses of {H} x {W} per step at focal ' +
            (f'{focal:.2f} .. {2 * focal:.2f}' if rand_focal else f'{focal:.2f}') + where +
            f', seed {src.seed}, ' + (f'watched every {src.watch_every} steps' if src.watch_every else 'not watched'))
    return src, what

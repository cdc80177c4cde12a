"""CPU / gloo: the precision watch (efficient-nerf_amd/watch.py) -- check, agree between the ranks, step down, record, log, render again --
alone on a stub engine with the teacher's five rungs, and through two of its callers that need no device: create_data.create_rand on
one rank and on two gloo ranks, and OnlineTeacherSource.batch on two ranks of which one holds no rows.  The expected call sequences,
records and log lines of the two callers are literals taken from the loops as they were written out in each caller before they shared
watch.py; render_path's two watches need a device (tests/test_watch_gpu.py)."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from test_create_data_cpu import FakeTeacher, _digest, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = ('fp16x1', 'fp16_fp8', 'fp16_mix', 'fp16x3_asm', 'fp16x3')
MISS = {'rgb_map': 0.5}


class LadderTeacher(FakeTeacher):
    """FakeTeacher with NeRFEngine's five rungs: what it renders depends on the rung, spot_check fails the first `misses` times, every
    call is logged with the rung it ran in (`origins`: the first ray origin of every render, i.e. which pose it was)"""
    LADDER = LADDER
    WATCH_RAYS = 4

    def __init__(self, misses=0, mode=0):
        self.mode, self.misses = mode, misses
        self.calls, self.origins = [], []

    @property
    def precision_name(self):
        return self.LADDER[self.mode]

    def render_rays(self, rays_o, rays_d):
        self.calls.append(('render', self.mode))
        self.origins.append(tuple(rays_o[0].tolist()) if len(rays_o) else None)
        return {'rgb_map': super().render_rays(rays_o, rays_d)['rgb_map'] + 0.01 * self.mode}

    def spot_check(self, ro, rd, got):
        self.calls.append(('check', self.mode))
        assert torch.equal(got['rgb_map'], FakeTeacher.render_rays(self, ro, rd)['rgb_map'] + 0.01 * self.mode)   # what was just rendered for these rays
        if self.misses > 0:
            self.misses -= 1
            return False, dict(MISS)
        return True, {'rgb_map': 0.}

    def step_down(self):
        self.calls.append(('step_down', self.mode))
        self.mode = min(self.mode + 1, len(self.LADDER) - 1)
        return self.precision_name


# ---- the shared loop alone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('misses', [0, 1, 2, 3, 4, 5])
def test_the_loop_walks_the_ladder_and_stops_on_its_last_rung(pkg, misses):
    """a teacher frame watched as render_path watches it: every miss is one step down, one record, one line and one render; the rung
    after the fourth miss has no fast mode left, so it is rendered and neither checked nor stepped from -- five misses are four"""
    from efficient_nerf_amd.watch import Watch
    eng, lines = LadderTeacher(misses), []
    ro, rd = torch.rand(6, 3), torch.rand(6, 3)
    w = Watch(len(eng.LADDER), log=lines.append)

    def step_down(ok, d):
        was, now = eng.precision_name, eng.step_down()
        return {'frame': 7, 'from': was, 'to': now, 'diffs': d}, f'[precision] frame 7: {was} is {d} -> {now}; frame rendered again'

    got = w.run(eng.render_rays(ro, rd), check=lambda got: eng.spot_check(ro, rd, got), step_down=step_down, again=lambda: eng.render_rays(ro, rd),
                live=lambda: eng.precision_name != 'fp16x3')
    n = min(misses, 4)
    want = [('render', 0)]
    for k in range(n):
        want += [('check', k), ('step_down', k), ('render', k + 1)]
    if n < 4:
        want += [('check', n)]
    assert eng.calls == want
    assert torch.equal(got['rgb_map'], FakeTeacher.render_rays(eng, ro, rd)['rgb_map'] + 0.01 * n) and eng.precision_name == LADDER[n]
    assert w.fallbacks == [{'frame': 7, 'from': LADDER[k], 'to': LADDER[k + 1], 'diffs': MISS} for k in range(n)]
    assert lines == [f"[precision] frame 7: {LADDER[k]} is {{'rgb_map': 0.5}} -> {LADDER[k + 1]}; frame rendered again" for k in range(n)]
    assert w.checks == min(n + 1, 4) and w.worst == (MISS if n else {'rgb_map': 0.})
    assert w.stats() == {'checks': w.checks, 'fallbacks': w.fallbacks, 'worst': w.worst}


def test_the_loop_without_a_check_on_this_rank_counts_none_and_a_number_is_a_maximum(pkg):
    """check() -> None: nothing to check on this rank (good, not counted); a check that reports one number keeps its maximum; a caller
    that returns no line logs nothing; max_steps bounds a check that never passes"""
    from efficient_nerf_amd.watch import Watch
    lines, renders = [], []
    w = Watch(6, log=lines.append, worst=0.0)
    assert w.run('a', check=lambda got: None, step_down=None, again=None) == 'a' and w.stats() == {'checks': 0, 'fallbacks': [], 'worst': 0.0}
    diffs = iter([0.25, 0.75, 0.5, 0.1, 0.1, 0.1, 0.1])
    got = w.run(0, check=lambda got: (False, next(diffs)), step_down=lambda ok, d: ({'n': len(renders), 'ok': ok, 'diff': d}, None),
                again=lambda: renders.append(1) or len(renders))
    assert got == 6 and w.checks == 6 and w.worst == 0.75 and [f['n'] for f in w.fallbacks] == list(range(6)) and not lines
    assert all(f['ok'] is False for f in w.fallbacks)


# ---- create_rand ---------------------------------------------------------------------------------------------------------------------------
H, W, SPLIT = 6, 8, 64


def _create(rank, world, port, out_dir, n_pose, i_save, misses, mode, watch, res_dir=None):
    """one rank of create_rand on a LadderTeacher; returns (and, spawned, saves) the engine's calls and origins, timings and the log"""
    sys.path.insert(0, ROOT)
    import _pkg
    _pkg.load()
    from efficient_nerf_amd import dist as D
    from efficient_nerf_amd.create_data import RandStream, create_rand
    from oracle import r2l_oracle as O
    if world > 1:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
        D.init(backend='gloo')
    eng, lines, tm = LadderTeacher(misses[rank], mode), [], {}
    n = create_rand(eng, H, W, O.focal_from_angle(W), n_pose, out_dir, i_save=i_save, split_size=SPLIT, stream=RandStream(), log=lines.append,
                    get_rays_fn=lambda H, W, focal, c2w, device=None: O.get_rays(H, W, focal, c2w), timings=tm, watch=watch)
    assert n == (n_pose // i_save) * (i_save * H * W // SPLIT)
    res = {'calls': eng.calls, 'origins': eng.origins, 'watch': tm.get('watch'), 'lines': lines, 'mode': eng.precision_name}
    if world > 1:
        import torch.distributed as dist
        torch.save(res, os.path.join(res_dir, f'r{rank}.pt'))
        dist.destroy_process_group()
    return res


def test_create_rand_on_one_rank_renders_only_the_missed_pose_again(tmp_path):
    d, d_final = str(tmp_path / 'missed'), str(tmp_path / 'final')
    res = _create(0, 1, 0, d, 4, 2, [1], 0, True)
    assert res['calls'] == [('render', 0), ('check', 0), ('step_down', 0), ('render', 1), ('check', 1), ('render', 1),
                            ('render', 1), ('check', 1), ('render', 1)]
    o = res['origins']
    assert o[0] == o[1] and len(set(o)) == 4                   # pose 1 twice, poses 2, 3, 4 once each
    assert res['watch'] == {'checks': 3, 'fallbacks': [{'pose': 1, 'from': 'fp16x1', 'to': 'fp16_fp8', 'diffs': {'rgb_map': 0.5}}],
                            'worst': {'rgb_map': 0.5}, 'precision': 'fp16_fp8'}
    assert res['lines'] == ["[precision] pose 1: fp16x1 is {'rgb_map': 0.5} from fp16x3 on 4 of its rays -> fp16_fp8; rendered again",
                            f'[2/4] Saved data at "{d}"', f'[4/4] Saved data at "{d}"']
    final = _create(0, 1, 0, d_final, 4, 2, [0], 1, True)      # a run that starts in the mode the first one ended in
    assert final['calls'] == [('render', 1), ('check', 1), ('render', 1)] * 2 and final['watch']['fallbacks'] == []
    assert _digest(d) == _digest(d_final) and len(_digest(d)) == 2


def test_create_rand_unwatched_checks_nothing(tmp_path):
    res = _create(0, 1, 0, str(tmp_path / 'd'), 4, 2, [1], 0, False)
    assert res['calls'] == [('render', 0)] * 4 and res['watch'] is None and res['mode'] == 'fp16x1'
    assert not any('[precision]' in ln for ln in res['lines'])


@pytest.fixture(scope='module')
def two_rank_group(tmp_path_factory):
    """two gloo ranks, save groups of three poses (rank 0 renders poses 1 and 3 of a group, rank 1 pose 2), rank 1's first check misses"""
    out = tmp_path_factory.mktemp('watch_two')
    os.makedirs(out / 'res')
    mp.spawn(_create, args=(2, _free_port(), str(out / 'w2'), 6, 3, [0, 1], 0, True, str(out / 'res')), nprocs=2, join=True)
    return [torch.load(out / 'res' / f'r{r}.pt', weights_only=False) for r in range(2)], str(out / 'w2')


@pytest.mark.timeout(120)
def test_create_rand_on_two_ranks_steps_down_together_and_renders_the_group_again(two_rank_group, tmp_path):
    (r0, r1), d2 = two_rank_group
    assert r0['calls'] == [('render', 0), ('check', 0), ('render', 0), ('step_down', 0), ('render', 1), ('check', 1), ('render', 1),
                           ('render', 1), ('check', 1), ('render', 1)]
    assert r1['calls'] == [('render', 0), ('check', 0), ('step_down', 0), ('render', 1), ('check', 1), ('render', 1), ('check', 1)]
    assert r0['origins'][:2] == r0['origins'][2:4] and r1['origins'][0] == r1['origins'][1]      # each rank's share of group 1, twice
    assert r0['watch'] == {'checks': 3, 'fallbacks': [{'pose': 1, 'from': 'fp16x1', 'to': 'fp16_fp8', 'diffs': "another rank's pose"}],
                           'worst': {'rgb_map': 0.0}, 'precision': 'fp16_fp8'}
    assert r1['watch'] == {'checks': 3, 'fallbacks': [{'pose': 1, 'from': 'fp16x1', 'to': 'fp16_fp8', 'diffs': {'rgb_map': 0.5}}],
                           'worst': {'rgb_map': 0.5}, 'precision': 'fp16_fp8'}
    assert r0['lines'] == ["[precision] pose 1: fp16x1 is another rank's pose from fp16x3 on 4 of its rays -> fp16_fp8; rendered again",
                           f'[3/6] Saved data at "{d2}"', f'[6/6] Saved data at "{d2}"']
    assert r1['lines'] == ["[precision] pose 1: fp16x1 is {'rgb_map': 0.5} from fp16x3 on 4 of its rays -> fp16_fp8; rendered again",
                           f'[3/6] Saved data at "{d2}"', f'[6/6] Saved data at "{d2}"']
    d1 = str(tmp_path / 'w1')
    _create(0, 1, 0, d1, 6, 3, [1], 0, True)
    assert _digest(d1) == _digest(d2) and len(_digest(d2)) == 4


# ---- OnlineTeacherSource.batch: a rank without rows beside a rank that misses -----------------------------------------------------------
def _online(rank, world, port, res_dir):
    sys.path.insert(0, ROOT)
    import _pkg
    _pkg.load()
    import torch.distributed as dist
    from efficient_nerf_amd import dist as D
    from test_online_cpu import _source
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    D.init(backend='gloo')
    eng, lines = LadderTeacher(1 if rank == 0 else 0), []
    src = _source(eng, lines.append, watch_every=10)
    ro, rd, target = src.batch(10, 1, rows=D.row_shard(1, rank, world))      # one ray: rank 0 holds it, rank 1 holds nothing
    torch.save({'calls': eng.calls, 'lines': lines, 'checks': src.checks, 'fallbacks': src.fallbacks, 'target': target,
                'want': FakeTeacher.render_rays(eng, ro, rd)['rgb_map'] + 0.01}, os.path.join(res_dir, f'r{rank}.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_online_rank_without_rows_enters_every_collective_and_counts_it_as_a_check(pkg, tmp_path):
    mp.spawn(_online, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f'r{r}.pt', weights_only=False) for r in range(2))
    assert r0['calls'] == [('render', 0), ('check', 0), ('step_down', 0), ('render', 1), ('check', 1)]
    assert r1['calls'] == [('step_down', 0)]                   # no rows: nothing rendered, nothing checked, the rung followed
    assert r0['checks'] == r1['checks'] == 2
    assert r0['fallbacks'] == [{'step': 10, 'from': 'fp16x1', 'to': 'fp16_fp8', 'diffs': {'rgb_map': 0.5}}]
    assert r1['fallbacks'] == [{'step': 10, 'from': 'fp16x1', 'to': 'fp16_fp8', 'diffs': {}}]
    assert r0['lines'] == ["[precision] step 10: fp16x1 is {'rgb_map': 0.5} from fp16x3 on 4 of the batch's rays -> fp16_fp8; batch rendered again"]
    assert r1['lines'] == []                                   # one line per run: rank 0's
    assert torch.equal(r0['target'], r0['want']) and torch.equal(r1['target'], r0['target'])

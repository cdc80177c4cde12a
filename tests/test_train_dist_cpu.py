"""CPU: what a ray-sharded training run decides on the host (efficient-nerf_amd/dist.py, train.py, frontend.py): the slices and the
weights of the ordered gradient sum, --dist_seed, the refusal of more ranks than rays, and the start-up seed that makes every
rank's host and device draws the same (two gloo ranks)."""
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('n', [0, 1, 37])
@pytest.mark.parametrize('world', [1, 2, 3, 8])
def test_slices_and_weights(pkg, n, world):
    from efficient_nerf_amd import dist as D
    bounds, weights = D.shard_weights(n, world)
    assert len(bounds) == len(weights) == world
    assert bounds[0][0] == 0 and bounds[-1][1] == n and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))      # contiguous, complete
    sizes = [b - a for a, b in bounds]
    assert sum(sizes) == n and all(s >= 0 for s in sizes) and max(sizes) - min(sizes) <= 1
    assert bounds == [D.row_shard(n, r, world) for r in range(world)]
    assert weights == [(s / n if n else 0.) for s in sizes]
    if n:
        assert abs(sum(weights) - 1.) <= 1e-15 * world
    if n == 37 and world == 2:
        assert sizes == [19, 18]
    if n == 1:
        assert sizes == [1] + [0] * (world - 1) and weights[0] == 1.


def test_sum_parts_checks_its_arguments(pkg, built_lib):
    """r2l_train_sum_parts refuses a bad call with a code and a message before any device is touched"""
    import ctypes as C
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    assert 'r2l_train_sum_parts' in _lib.SIGNATURES
    w = (C.c_float * 65)(*([1.0] * 65))
    p, q = C.c_void_p(0x1000), C.c_void_p(0x9000)
    err = lambda: L.r2l_last_error().decode()
    for n_part in (0, -1, 65):
        assert L.r2l_train_sum_parts(p, 16, n_part, w, 8, q, None) == -1 and 'r2l_train_sum_parts' in err() and '64' in err()
    assert L.r2l_train_sum_parts(p, 16, 2, None, 8, q, None) == -1                       # no weights
    assert L.r2l_train_sum_parts(p, 16, 2, w, -1, q, None) == -1
    assert L.r2l_train_sum_parts(None, 16, 2, w, 8, q, None) == -1 and L.r2l_train_sum_parts(p, 16, 2, w, 8, None, None) == -1
    assert L.r2l_train_sum_parts(p, 4, 2, w, 8, q, None) == -1                           # parts would overlap each other
    assert L.r2l_train_sum_parts(p, 16, 2, w, 8, C.c_void_p(0x1000 + 16), None) == -1 and 'overlaps' in err()


def test_dist_seed_parses(pkg):
    from efficient_nerf_amd.frontend import parse_args
    assert parse_args([]).dist_seed == -1
    assert parse_args(['--dist_seed', '5']).dist_seed == 5
    with pytest.raises(SystemExit):
        parse_args(['--dist_seed', 'five'])


def test_more_ranks_than_rays_is_refused_in_one_line(pkg):
    from efficient_nerf_amd import train as T
    T.refuse_more_ranks_than_rays(1, 1)
    T.refuse_more_ranks_than_rays(8, 8)
    with pytest.raises(SystemExit) as e:
        T.refuse_more_ranks_than_rays(8, 7)
    msg = str(e.value)
    assert '8 ranks' in msg and '7 rays' in msg and '\n' not in msg


def test_one_rank_seeds_nothing(pkg):
    from efficient_nerf_amd import dist as D
    np.random.seed(3)
    torch.manual_seed(3)
    a, b = np.random.get_state()[1].copy(), torch.random.get_rng_state().clone()
    assert D.seed_all(5) is None and D.rank_world() == (0, 1)
    assert np.array_equal(np.random.get_state()[1], a) and torch.equal(torch.random.get_rng_state(), b)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _seed_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    import _pkg
    _pkg.load()
    import torch.distributed as dist
    from efficient_nerf_amd import dist as D
    torch.set_num_threads(1)
    D.init(backend='gloo')
    np.random.seed(100 + rank)              # the ranks start from different streams, as fresh processes do
    torch.manual_seed(200 + rank)
    res = {}
    for name, given in (('drawn', None), ('drawn_minus_one', -1), ('given', 5)):
        before = np.random.RandomState(100).randint(0, 2 ** 31 - 1) if name == 'drawn' else None
        seed = D.seed_all(given)
        res[name] = (seed, np.random.permutation(50).tolist(), torch.rand(8), before)
    torch.save(res, os.path.join(out_dir, f's{rank}.pt'))
    D.barrier_sync()
    dist.destroy_process_group()


def test_two_ranks_agree_on_the_seed_and_draw_the_same(tmp_path):
    ctx = mp.spawn(_seed_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    t_end = time.monotonic() + 120
    try:
        while not ctx.join(timeout=0.5):                                 # raises when a rank failed, and stops the other
            assert time.monotonic() < t_end, 'the two ranks did not finish in 120 s'
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    r = [torch.load(os.path.join(str(tmp_path), f's{k}.pt'), weights_only=False) for k in range(2)]
    for name in ('drawn', 'drawn_minus_one', 'given'):
        a, b = r[0][name], r[1][name]
        assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]), name
    assert r[0]['given'][0] == 5
    assert r[0]['drawn'][0] == r[0]['drawn'][3]                      # the default: a draw from rank 0's own stream
    assert r[0]['drawn'][1] != r[0]['given'][1]
    # the draws are those of one process seeded with that seed
    np.random.seed(5)
    torch.manual_seed(5)
    assert np.random.permutation(50).tolist() == r[0]['given'][1] and torch.equal(torch.rand(8), r[0]['given'][2])

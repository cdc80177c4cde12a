"""GPU: the training kernels (csrc/r2l_train.hip, csrc/nerf_train.hip) past their second-level loop edges: the g_W reduction once the
slab count is capped and slabs stay empty, the loss once its final pass walks the partial sums twice, the gradient sum once its
grid-stride loop goes round again, the scan's backward pass with a ragged chunk behind full ones, Adam and the element-wise pass
at their tails and on column slices, and one whole step above 65,536 rays; and (section 8) NaN and infinity through the scan's
backward pass, the element-wise pass, the loss and Adam, against torch autograd and torch.optim.Adam on the CPU.

Yardsticks, none of them new: float64 on the CPU with the derived rounding bounds of tests/test_train_gpu.py (gamma_m), torch's
own fp32 mul and add on the device where the kernel promises those bits (tests/test_train_dist_gpu.py), and float64 autograd of
oracle/r2l_oracle.py with the band torch's fp32 keeps from it (factor 4) where ReLUs or the scan are crossed.

What each case is there to reach is computed in Python from the rules the kernels document (slab_rule, loss_partials,
sum_parts_items) and asserted by check_preconditions() when this file is imported, so that collecting it on a machine without
a GPU already tells whether the shapes still reach the paths; the tests compare the rules with the library where it exports them."""
import ctypes as C

import numpy as np
import pytest
import torch

from nonfinite_cases import INF, NAN, SCAN_N as SPECIAL_N, SCAN_S as SPECIAL_S, poisoned_rays, same_bits, same_masks, scan_combos, scan_reference

pytestmark = pytest.mark.gpu
U = 2.0 ** -24          # fp32 unit roundoff


def gamma(m):
    return m * U / (1 - m * U)


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


def _same_bits(a, b):
    """equal shapes and equal bit patterns (NaNs included, which torch.equal never calls equal)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- what the shapes below are chosen to reach, from the kernels' documented rules ---------------------------------------------
GW_SLAB_RAYS, GW_MAX_SLABS, GW_STAGE = 512, 128, 32          # r2l_train.hip: rays per slab, the cap, the k stage a slab is rounded to
LOSS_BLOCK = 256                                             # rays per partial sum, and the stride of the final pass
SUM_BLOCK, SUM_MAX_BLOCKS = 256, 2048                        # r2l_train_sum_parts' grid cap
SCAN_CHUNK = 64                                              # samples a wave holds at a time in the scan's backward pass

GEMM_BIG = [(65_537, 70, 130), (70_001, 8, 3), (98_304, 33, 129)]
LOSS_N = [256, 257, 65_536, 65_537, 70_001]
SUM_CASES = [(524_289, 1), (2_097_157, 0), (4_194_309, 0)]   # (count, base offset in floats: 1 breaks the 16-byte alignment)
SCAN_S = [63, 65, 100, 129, 257]
SCAN_N = [1, 3, 203]
STEP_RAYS = 70_001


def slab_rule(n):
    """(slabs, rays per slab, the slabs that hold no ray) of r2l_train_grad_weight: ceil(n / 512) slabs until 128, then 128 slabs of
    ceil(n / 128) rays rounded up to a multiple of 32"""
    if n <= 0:
        return 0, 0, []
    slabs = min(-(-n // GW_SLAB_RAYS), GW_MAX_SLABS)
    rays = -(-(-(-n // slabs)) // GW_STAGE) * GW_STAGE
    return slabs, rays, [k for k in range(slabs) if k * rays >= n]


def loss_partials(n):
    """(partial sums of r2l_train_mse_loss, trips of the final pass's loop on its busiest thread)"""
    n_partial = -(-n // LOSS_BLOCK)
    return n_partial, -(-n_partial // LOSS_BLOCK)


def sum_parts_items(count, base, pitch, n_part=3):
    """(float4 items, scalar items, trips of the grid-stride loop) of r2l_train_sum_parts for parts that start `base` floats behind a
    16-byte boundary"""
    aligned = base % 4 == 0 and (n_part == 1 or pitch % 4 == 0)
    n_vec = count // 4 if aligned else 0
    n_item = n_vec + (count - 4 * n_vec)
    return n_vec, count - 4 * n_vec, -(-n_item // (SUM_BLOCK * SUM_MAX_BLOCKS))


def _pitch4(count):
    return count + (-count) % 4


def check_preconditions():
    # 1. slabs: capped everywhere, empty ones at 65,537 (and 70,001), none at 98,304
    assert slab_rule(8192) == (16, 512, [])                                  # the largest shape the older tests run
    for n, _, _ in GEMM_BIG:
        assert n > GW_SLAB_RAYS * GW_MAX_SLABS and slab_rule(n)[0] == GW_MAX_SLABS
    assert slab_rule(65_537) == (128, 544, list(range(121, 128)))
    assert len(slab_rule(70_001)[2]) >= 1
    assert slab_rule(98_304) == (128, 768, [])
    assert slab_rule(STEP_RAYS)[0] == GW_MAX_SLABS
    # 3. the final pass of the loss: one full round at 65,536, a second one behind it
    assert [loss_partials(n)[1] for n in LOSS_N] == [1, 1, 1, 2, 2] and loss_partials(65_536)[0] == LOSS_BLOCK
    # 4. more than one grid: scalar path twice, vector path twice (with a scalar tail item), vector path three times
    grid = SUM_BLOCK * SUM_MAX_BLOCKS
    want = [(0, 524_289, 2), (524_289, 1, 2), (1_048_577, 1, 3)]
    for (count, base), w in zip(SUM_CASES, want):
        assert sum_parts_items(count, base, _pitch4(count)) == w
        assert (count // 4 if w[0] else count) > grid
    # 5. a ragged chunk behind at least one full one, but for S = 63 (one ragged chunk alone, the neighbour of 65)
    assert all(S % SCAN_CHUNK != 0 for S in SCAN_S) and [S // SCAN_CHUNK for S in SCAN_S] == [0, 1, 1, 2, 4]
    # 2. the sweep: all three sizes one past a tile edge together, and every drawn value inside the sets
    assert (129, 65, 129) in SWEEP and len(SWEEP) == 24 and len(set(SWEEP)) == 24
    assert all(n in SWEEP_N and i in SWEEP_IN and o in SWEEP_OUT for n, i, o in SWEEP)
    return True


SWEEP_N = [1, 31, 33, 127, 129, 511, 513, 1025]
SWEEP_IN = [1, 31, 33, 63, 65, 127, 129, 7, 61, 67, 131, 251]        # ... plus primes
SWEEP_OUT = [1, 2, 31, 33, 127, 129, 130, 257]


def _sweep():
    rng = np.random.RandomState(7)
    cases = [(129, 65, 129)]
    while len(cases) < 24:
        c = (int(rng.choice(SWEEP_N)), int(rng.choice(SWEEP_IN)), int(rng.choice(SWEEP_OUT)))
        if c not in cases:
            cases.append(c)
    return cases


SWEEP = _sweep()
check_preconditions()


# ---- 1. and 2. the two backward GEMMs ------------------------------------------------------------------------------------------
def _place(vals, strided, extra):
    """vals [n, w] on the device: contiguous, or as the window (row 1, column 3) of a NaN-filled parent [n + 2, w + extra].
    Returns (the [n, w] view, the parent, the row pitch)."""
    n, w = vals.shape
    if not strided:
        t = vals.cuda()
        return t, t, w
    parent = torch.full((n + 2, w + extra), NAN, device='cuda')
    view = parent[1:n + 1, 3:3 + w]
    view.copy_(vals)
    return view, parent, w + extra


def _only_the_window_changed(parent, keep, view_shape, strided):
    """every element of the parent outside the window holds the bits it held before the call"""
    if not strided:
        return True
    n, w = view_shape
    after = parent.clone()
    after[1:n + 1, 3:3 + w] = keep[1:n + 1, 3:3 + w]
    return _same_bits(after, keep)


def _grad_weight(L, gz, ldz, x, ldx, n, out_dim, in_dim, with_bias=True, margin=16):
    """g_W and g_b as the trainers lay them out ([out * in | out] of one flat buffer), NaN before the call, between NaN margins and
    over a NaN workspace: (g_W, g_b or the untouched bias slot, the two margins, slabs)"""
    slabs = L.r2l_train_grad_weight_slabs(n)
    wn = out_dim * in_dim
    ws = torch.full((max(1, slabs * (wn + out_dim)),), NAN, device='cuda')
    flat = torch.full((margin + wn + out_dim + margin,), NAN, device='cuda')
    gw, gb = flat[margin:margin + wn], flat[margin + wn:margin + wn + out_dim]
    _check(L, L.r2l_train_grad_weight(_p(gz), ldz, _p(x), ldx, n, out_dim, in_dim, _p(gw), _p(gb) if with_bias else None, _p(ws),
                                      ws.numel(), _stream()))
    torch.cuda.synchronize()
    return gw.view(out_dim, in_dim), gb, torch.cat([flat[:margin], flat[margin + wn + out_dim:]]), slabs


def _gemm_case(L, n, in_dim, out_dim, strided, seed):
    """both backward GEMMs of one shape against float64 under the derived bounds; the ratios max err / bound (g_x, g_x accumulated,
    g_W, g_b) and what the g_W call left"""
    g = torch.Generator().manual_seed(seed)
    gz, x, w = torch.randn(n, out_dim, generator=g), torch.randn(n, in_dim, generator=g), torch.randn(out_dim, in_dim, generator=g) / 16
    c0 = torch.randn(n, in_dim, generator=g)
    gz_v, gz_p, ldz = _place(gz, strided, 5)
    x_v, x_p, ldx = _place(x, strided, 7)
    gz_keep, x_keep = gz_p.clone(), x_p.clone()
    wd = w.cuda()
    ratio = {}
    # g_x = g_z W, then on top of what the destination holds (one more addition)
    ref, mag = gz.double() @ w.double(), gz.double().abs() @ w.double().abs()
    for acc in (0, 1):
        gx_v, gx_p, ldgx = _place(c0 if acc else torch.full((n, in_dim), NAN), strided, 4 + acc)
        gx_keep = gx_p.clone()
        _check(L, L.r2l_train_grad_input(_p(gz_v), ldz, n, _p(wd), out_dim, in_dim, _p(gx_v), ldgx, acc, _stream()))
        torch.cuda.synchronize()
        want, scale = (ref + c0.double(), mag + c0.double().abs()) if acc else (ref, mag)
        bound = gamma(out_dim + 2 + acc) * scale
        d = (gx_v.cpu().double() - want).abs()
        ratio['g_x+' if acc else 'g_x'] = float((d / (bound + 1e-300)).max())
        assert torch.isfinite(gx_v).all() and bool((d <= bound).all()), (n, in_dim, out_dim, acc)
        assert _only_the_window_changed(gx_p, gx_keep, (n, in_dim), strided)
    # g_W = g_z^T x, g_b = column sums of g_z: a k-ordered fp32 chain over the rays plus one addition per slab
    gw, gb, margins, slabs = _grad_weight(L, gz_v, ldz, x_v, ldx, n, out_dim, in_dim)
    assert slabs == slab_rule(n)[0]
    m = n + slabs + 2
    refw, magw = gz.double().t() @ x.double(), gz.double().abs().t() @ x.double().abs()
    dw = (gw.cpu().double() - refw).abs()
    db = (gb.cpu().double() - gz.double().sum(0)).abs()
    ratio['g_W'] = float((dw / (gamma(m) * magw + 1e-300)).max())
    ratio['g_b'] = float((db / (gamma(m) * gz.double().abs().sum(0) + 1e-300)).max())
    print(f'n={n} {in_dim}->{out_dim}{" strided" if strided else ""}: {slabs} slabs, max err / bound: ' +
          ', '.join(f'{k} {v:.1e}' for k, v in ratio.items()))
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()              # a NaN from an unwritten slab of the workspace ends here
    assert bool((dw <= gamma(m) * magw).all()) and bool((db <= gamma(m) * gz.double().abs().sum(0)).all())
    assert torch.isnan(margins).all()
    gw2, gb2, _, _ = _grad_weight(L, gz_v, ldz, x_v, ldx, n, out_dim, in_dim)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)                      # two runs: the same bits
    assert _same_bits(gz_p, gz_keep) and _same_bits(x_p, x_keep)              # the inputs are read only
    return ratio, (gz_v, ldz, x_v, ldx, gw)


@pytest.mark.parametrize('n,in_dim,out_dim', GEMM_BIG)
def test_backward_gemms_past_the_slab_cap(L, n, in_dim, out_dim):
    """more than 65,536 rays: 128 slabs that grow, the last of them empty at 65,537 and 70,001 (their workgroups still write the
    zeros the slab pass adds) and none empty at 98,304; out_dim one and two past the 128-row tile, in_dim past 64 with a ragged ray
    tile.  |hip - f64| <= gamma_m (|g_z|^T |x|), m = n + slabs + 2; g_x under gamma_{out + 2} (+ 1 accumulated)."""
    check_preconditions()
    slabs, rays, empty = slab_rule(n)
    assert slabs == L.r2l_train_grad_weight_slabs(n) == GW_MAX_SLABS and rays > GW_SLAB_RAYS
    if n == 65_537:
        assert len(empty) >= 1
    if n == 98_304:
        assert empty == []
    _, (gz, ldz, x, ldx, gw) = _gemm_case(L, n, in_dim, out_dim, False, n + in_dim)
    # without a bias gradient: the same g_W bit for bit, and the slot a bias would take stays as it was
    gw_nb, slot, margins, _ = _grad_weight(L, gz, ldz, x, ldx, n, out_dim, in_dim, with_bias=False)
    assert torch.equal(gw_nb, gw)
    assert torch.isnan(slot).all() and torch.isnan(margins).all()
    # The bound grows with n, and one ray among 65,537 is below it: with g_z zero on every ray but the first and the last of the
    # last slab that holds rays, g_W and g_b are those two rays' alone, and a slab that loses its tail gives another answer.
    last = max(k for k in range(slabs) if k not in empty)
    rows = [last * rays, n - 1]
    assert rows[0] < n - 1 < (last + 1) * rays
    gz_m = torch.zeros_like(gz)
    gz_m[rows] = gz[rows]
    gw_m, gb_m, _, _ = _grad_weight(L, gz_m, ldz, x, ldx, n, out_dim, in_dim)
    z64, x64 = gz_m[rows].cpu().double(), x[rows].cpu().double()
    m = n + slabs + 2
    assert bool(((gw_m.cpu().double() - z64.t() @ x64).abs() <= gamma(m) * (z64.abs().t() @ x64.abs())).all())
    assert bool(((gb_m.cpu().double() - z64.sum(0)).abs() <= gamma(m) * z64.abs().sum(0)).all())
    assert gw_m.any() and gb_m.any()


@pytest.mark.parametrize('case', range(24))
def test_backward_gemms_seeded_shapes_at_the_tile_edges(L, case):
    """24 seeded (n, in_dim, out_dim) around the 128 x 64 x 32 tile, the odd cases as windows of wider NaN-filled buffers whose
    other elements keep their bits; the bounds of the test above"""
    n, in_dim, out_dim = SWEEP[case]
    _gemm_case(L, n, in_dim, out_dim, case % 2 == 1, 1000 + case)


# ---- 3. the loss past one round of partials ------------------------------------------------------------------------------------
def _margined(count, pad=32):
    """(a NaN-filled buffer, its middle `count` floats)"""
    buf = torch.full((pad + count + pad,), NAN, device='cuda')
    return buf, buf[pad:pad + count]


def _margins_are_nan(buf, count, pad=32):
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + count:]).all())


def _mse(L, rgb_d, tgt_d, n, through, with_err=True, finite=True):
    gbuf, gout = _margined(3 * n)
    ebuf, err = _margined(n)
    wbuf, ws = _margined(loss_partials(n)[0])                  # exactly ceil(n / 256) floats
    loss = torch.full((1,), NAN, device='cuda')
    _check(L, L.r2l_train_mse_loss(_p(rgb_d), _p(tgt_d), n, through, _p(gout), _p(err) if with_err else None, _p(loss), _p(ws),
                                   ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert _margins_are_nan(gbuf, 3 * n) and _margins_are_nan(ebuf, n) and _margins_are_nan(wbuf, ws.numel())
    assert not finite or torch.isfinite(ws).all()
    return loss, gout.view(n, 3), err


@pytest.mark.parametrize('through', [0, 1])
@pytest.mark.parametrize('n', LOSS_N)
def test_mse_loss_past_one_round_of_partials(L, n, through):
    """256 and 257 rays (one block exactly, one ray into the second), 65,536 (256 partials: the final pass's loop once, every thread
    busy), 65,537 and 70,001 (twice): loss within gamma_{n + 600}, gradient and per-ray error within gamma_8 of float64; a
    workspace of exactly ceil(n / 256) floats between NaN margins; without the per-ray error the same bits; twice the same bits"""
    g = torch.Generator().manual_seed(7 * n + through)
    rgb, tgt = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    rgb_d, tgt_d = rgb.cuda(), tgt.cuda()
    loss, gout, err = _mse(L, rgb_d, tgt_d, n, through)
    d = rgb.double() - tgt.double()
    mean = float((d ** 2).mean())
    want_g = 2 * d / (3 * n) * (rgb.double() * (1 - rgb.double()) if through else 1)
    want_e = (d ** 2).mean(1)
    r_loss = abs(loss.item() - mean) / (gamma(n + 600) * mean)
    r_g = float(((gout.cpu().double() - want_g).abs() / (gamma(8) * want_g.abs() + 1e-45)).max())
    r_e = float(((err.cpu().double() - want_e).abs() / (gamma(8) * want_e + 1e-45)).max())
    print(f'loss n={n} through_sigmoid={through}: {loss_partials(n)[0]} partials, max err / bound: loss {r_loss:.1e}, gradient {r_g:.3f}, '
          f'per-ray error {r_e:.3f}')
    assert abs(loss.item() - mean) <= gamma(n + 600) * mean
    assert bool(((gout.cpu().double() - want_g).abs() <= gamma(8) * want_g.abs() + 1e-45).all())
    assert bool(((err.cpu().double() - want_e).abs() <= gamma(8) * want_e + 1e-45).all())
    loss_n, gout_n, slot = _mse(L, rgb_d, tgt_d, n, through, with_err=False)
    assert torch.equal(loss_n, loss) and torch.equal(gout_n, gout) and torch.isnan(slot).all()
    loss_2, gout_2, err_2 = _mse(L, rgb_d, tgt_d, n, through)
    assert torch.equal(loss_2, loss) and torch.equal(gout_2, gout) and torch.equal(err_2, err)
    if loss_partials(n)[1] > 1:
        # One ray among 65,537 moves the mean by less than gamma_{n + 600}: with the first 65,536 rays on their targets the whole
        # loss sits in the partials of the second round, and a final pass that stops after one round gives 0 for it.
        first = LOSS_BLOCK * LOSS_BLOCK
        tgt_b = tgt.clone()
        tgt_b[:first] = rgb[:first]
        loss_b, _, _ = _mse(L, rgb_d, tgt_b.cuda(), n, through)
        mean_b = float(((rgb.double() - tgt_b.double()) ** 2).mean())
        print(f'loss n={n}: the rays behind {first} alone: {loss_b.item():.6e}, float64 {mean_b:.6e}')
        assert mean_b > 0 and abs(loss_b.item() - mean_b) <= gamma(n + 600) * mean_b


# ---- 4. the gradient sum past one grid -----------------------------------------------------------------------------------------
def _weight_sets(n_part):
    """n_r / n of n = 37 over the parts (no powers of two); a set with a zero weight (an empty slice) last and first"""
    split = lambda n, w: [(n // w + (1 if r < n % w else 0)) / n for r in range(w)]
    z = split(37, n_part - 1) + [0.0]
    return [split(37, n_part), z, [0.0] + z[:-1]]


def _values(shape, seed):
    """magnitudes over 1e-9 .. 1, every fourth value scaled by 1e-37: its products with the weights are denormal or flush to 0"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g).sign() * 10 ** (-9 * torch.rand(shape, generator=g))
    tiny = torch.rand(shape, generator=g) < 0.25
    return torch.where(tiny, v * 1e-37, v)


@pytest.mark.parametrize('count,base', SUM_CASES)
def test_sum_parts_past_one_grid(L, count, base):
    """three parts, more items than 2,048 x 256 threads take in one trip: element by element on an unaligned base (2 trips), in
    float4 with a scalar item behind them (2 trips, 3 trips); out beside the parts and out = part 0, where a part read after part 0
    was overwritten would show.  torch's mul and add on the device, bit for bit; nothing behind `count`, no other part touched."""
    n_part, pitch = 3, _pitch4(count)
    n_vec, n_tail, trips = sum_parts_items(count, base, pitch)
    assert (n_vec if n_vec else count) > SUM_BLOCK * SUM_MAX_BLOCKS and trips >= 2          # the loop runs more than once
    src = _values((n_part, count), count).cuda()
    for wi, weights in enumerate(_weight_sets(n_part)):
        wt = torch.tensor(weights, dtype=torch.float32)                      # the fp32 the kernel receives by value
        wd = wt.cuda()
        acc = src[0] * wd[0]
        for r in range(1, n_part):
            acc = acc + src[r] * wd[r]
        if wi == 0:
            prod = src * wd[:, None]                                         # denormal products are among the values added
            assert bool(((prod != 0) & (prod.abs() < 1.17e-38)).any())
            del prod
        for alias in (False, True):
            buf = torch.full((base + n_part * pitch + count + 8,), -7., device='cuda')
            parts = buf[base:]
            assert parts.data_ptr() % 16 == 4 * (base % 4)
            for k in range(n_part):
                parts[k * pitch:k * pitch + count] = src[k]
            keep = buf.clone()
            out = parts if alias else torch.full((count + 8,), -7., device='cuda')
            w = (C.c_float * n_part)(*wt.tolist())
            _check(L, L.r2l_train_sum_parts(_p(parts), pitch, n_part, w, count, _p(out), _stream()))
            torch.cuda.synchronize()
            assert torch.equal(out[:count], acc), (count, base, wi, alias)
            if alias:
                keep[base:base + count] = acc
            else:
                assert bool((out[count:] == -7.).all())
            assert torch.equal(buf, keep)
            del buf, keep, out


# ---- 5. the scan's backward pass with a ragged chunk behind full ones ----------------------------------------------------------
def _scan_case(n, S, kind, seed):
    """tests/test_train_teacher_gpu.py's recipe: raw [n,S,4], per-ray sorted z [n,S], rays_d [n,3], g_rgb_map [n,3]; 'thin'
    (densities N(0.6, 2)), 'mixed' (N(0, 1) ... N(0, 300)), 'empty' (no positive density), 'saturated' (a stretch with sigma = 300
    ... 3000, alpha = 1 in fp32): here the stretch is samples 60 .. 67, across the edge between the first two chunks, where the
    ray has them (at S = 63 it stays where the recipe puts it, in the interior)"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, S, 4, generator=g)
    scale = 10 ** (2.5 * torch.rand(n, 1, generator=g))
    raw[..., 3] = raw[..., 3] * scale + 0.3 * scale
    if kind == 'thin':
        raw[..., 3] = 2. * torch.randn(n, S, generator=g) + 0.6
    if kind == 'empty':
        raw[..., 3] = -raw[..., 3].abs() - 0.5
    if kind == 'saturated':
        a, b = (60, min(68, S)) if S > SCAN_CHUNK else (S // 3, S // 3 + max(1, S // 8))
        raw[:, a:b, 3] = 300. * (1 + 9 * torch.rand(n, 1, generator=g))
    z = torch.sort(2. + 4. * torch.rand(n, S, generator=g), -1)[0]
    rd = torch.randn(n, 3, generator=g)
    g_rgb = torch.randn(n, 3, generator=g)
    return raw, z, rd, g_rgb


def _scan_autograd(O, raw, z, rd, g_rgb, white, noise, dtype):
    r = raw.to(dtype).clone().requires_grad_(True)
    nz = None if noise is None else noise.to(dtype)
    rgb = O.raw2outputs(r, z.to(dtype), rd.to(dtype), white_bkgd=white, noise=nz)[0]
    (rgb * g_rgb.to(dtype)).sum().backward()
    return r.grad.detach()


def _scan_hip(L, raw, z, rd, g_rgb, white, noise, pad=64):
    """g_raw written into the middle of a NaN-filled buffer: (g_raw, the buffer's two margins)"""
    n, S = z.shape
    buf = torch.full((pad + n * S * 4 + pad,), NAN, device='cuda')
    dev = [t.cuda().contiguous() for t in (raw, z, rd, g_rgb)]
    nz = None if noise is None else noise.cuda().contiguous()
    out = buf[pad:pad + n * S * 4]
    _check(L, L.nerf_train_raw2outputs_backward(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(nz), n, S, int(white), _p(dev[3]), _p(out), _stream()))
    torch.cuda.synchronize()
    return out.view(n, S, 4).cpu(), torch.cat([buf[:pad], buf[pad + n * S * 4:]]).cpu()


def _rel(got, ref, dim=None):
    """relative L2 gap, whole or per ray (dim = the dimensions summed over); 0 / 0 = 0"""
    d, r = (got.double() - ref.double()) ** 2, ref.double() ** 2
    num, den = (d.sum().sqrt(), r.sum().sqrt()) if dim is None else (d.sum(dim).sqrt(), r.sum(dim).sqrt())
    q = torch.where(den > 0, num / den, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float('inf'))))
    return float(q.max())


@pytest.mark.parametrize('n', SCAN_N)
@pytest.mark.parametrize('S', SCAN_S)
def test_scan_backward_with_a_ragged_last_chunk(L, S, n):
    """S = 65, 100, 129, 257: the carry enters pass 2 from a partly filled last chunk, whose lanes behind the ray's end must add
    nothing to it (and be the factor 1 in pass 1's running product); S = 63: that chunk alone; 1 ray, 3 rays (a workgroup of 4
    waves not filled) and 203.  As
    test_scan_backward_against_float64: within 4 x torch-fp32's gap from float64 autograd, finite, exactly 0 where it must be, the
    same bits twice, nothing written beside [n, S, 4]."""
    from oracle import r2l_oracle as O
    for kind in ('thin', 'mixed', 'saturated', 'empty'):
        for white in (False, True):
            for with_noise in (False, True):
                seed = S * 8 + 4 * white + 2 * with_noise + 4096 * n
                raw, z, rd, g_rgb = _scan_case(n, S, kind, seed)
                noise = torch.randn(n, S, generator=torch.Generator().manual_seed(seed + 1)) if with_noise else None
                if kind == 'empty' and noise is not None:
                    noise = -noise.abs()
                got, margins = _scan_hip(L, raw, z, rd, g_rgb, white, noise)
                again, _ = _scan_hip(L, raw, z, rd, g_rgb, white, noise)
                ref = _scan_autograd(O, raw, z, rd, g_rgb, white, noise, torch.float64)
                t32 = _scan_autograd(O, raw, z, rd, g_rgb, white, noise, torch.float32)
                gap_hip, gap_t32 = _rel(got, ref), _rel(t32, ref)
                ray_hip, ray_t32 = _rel(got, ref, (1, 2)), _rel(t32, ref, (1, 2))
                if not np.isfinite(gap_t32):
                    gap_t32 = float('inf')
                if not np.isfinite(ray_t32):
                    ray_t32 = float('inf')
                print(f'S={S} n={n} {kind} white={white} noise={with_noise}: relative L2 gap from float64: HIP {gap_hip:.2e}, torch fp32 '
                      f'{gap_t32:.2e}; worst ray: HIP {ray_hip:.2e}, torch fp32 {ray_t32:.2e}')
                assert torch.isfinite(got).all()
                assert torch.isnan(margins).all()                                   # nothing written outside [n, S, 4]
                assert torch.equal(got, again)                                      # the same bits from run to run
                pre = raw[..., 3] + (noise if noise is not None else 0.)
                assert not got[..., 3][pre <= 0].any()                              # relu'(0) = 0: exactly zero
                assert not got[:, -1, 3].any()                                      # the last sample: exp(-sigma 1e10) = 0 or sigma = 0
                if kind == 'empty':
                    assert not got.any() and not ref.any()
                assert gap_hip <= 4 * gap_t32, (kind, white, with_noise, gap_hip, gap_t32)


# ---- 6. Adam and the element-wise pass at their tails --------------------------------------------------------------------------
def _torch_adam_run(p0, grads, lrs, dtype):
    prm = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adam([prm], lr=1.0, betas=(0.9, 0.999))
    for gr, lr in zip(grads, lrs):
        opt.param_groups[0]['lr'] = lr
        prm.grad = gr.to(dtype).clone()
        opt.step()
    return prm.detach()


@pytest.mark.parametrize('count', [1, 255, 257, 4099])
def test_adam_at_the_tail_of_a_block(L, count):
    """1, one short of a block, one into the second, 4,099: 5 steps, gradient magnitudes over 1e-9 ... 1, another lr every step,
    no further from torch's float64 Adam than 4 x torch's own fp32 Adam is; parameters, moments and gradient between NaN margins
    that stay NaN"""
    g = torch.Generator().manual_seed(11 + count)
    p0 = torch.randn(count, generator=g)
    mags = 10 ** (-9 * torch.rand(count, generator=g))
    grads = [torch.randn(count, generator=g) * mags for _ in range(5)]
    lrs = [1e-4 + 4e-5 * k for k in range(5)]
    p64 = _torch_adam_run(p0, grads, lrs, torch.float64)
    p32 = _torch_adam_run(p0, grads, lrs, torch.float32)
    (pb, p), (mb, m), (vb, v), (gb, gr_d) = (_margined(count) for _ in range(4))
    p.copy_(p0)
    m.zero_()
    v.zero_()
    for k, (gr, lr) in enumerate(zip(grads, lrs)):
        gr_d.copy_(gr)
        _check(L, L.r2l_train_adam(_p(p), _p(gr_d), _p(m), _p(v), count, lr, k + 1, _stream()))
    torch.cuda.synchronize()
    gap_hip = float((p.cpu().double() - p64).abs().max())
    gap_t32 = float((p32.double() - p64).abs().max())
    print(f'Adam count={count}: max|p_hip - p_f64| = {gap_hip:.3e}, max|p_torch_fp32 - p_f64| = {gap_t32:.3e}')
    assert all(_margins_are_nan(b, count) for b in (pb, mb, vb, gb))
    assert torch.equal(gr_d.cpu(), grads[-1]) and torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all()
    assert gap_hip <= 4 * gap_t32


ACT_PITCH = dict(g_y=64, y=66, post=72, g_z=68, g_res=80, g_post=96)


@pytest.mark.parametrize('act', ['none', 'relu', 'lrelu', 'sigmoid'])
def test_act_backward_on_column_slices(L, act):
    """width 50 as windows of six buffers of six different pitches (64 ... 96), as the trainer's column slices of wider buffers:
    the gamma_4 bounds of test_act_backward_against_float64, and outside the 50 columns every buffer keeps its bits"""
    code = {'none': 0, 'relu': 1, 'lrelu': 2, 'sigmoid': 3}[act]
    g = torch.Generator().manual_seed(40 + code)
    n, w, scale = 301, 50, 0.5
    u = torch.randn(n, w, generator=g)
    a = {'none': u, 'relu': torch.relu(u), 'lrelu': torch.nn.functional.leaky_relu(u), 'sigmoid': torch.sigmoid(u)}[act]
    gy = torch.randn(n, w, generator=g)
    for with_post in ((False, True) if act != 'sigmoid' else (False,)):
        post = torch.randn(n, w, generator=g) if with_post else None
        y = a + post if with_post else a
        a64 = y.double() - post.double() if with_post else y.double()
        d64 = {'none': torch.ones_like(a64), 'relu': (a64 > 0).double(), 'lrelu': torch.where(a64 > 0, 1.0, 0.01).double(), 'sigmoid': a64 * (1 - a64)}[act]
        gu64 = gy.double() * d64
        res0, post0 = torch.randn(n, w, generator=g), torch.randn(n, w, generator=g)
        for res_acc in (0, 1):
            bufs = {}
            for name, vals in (('g_y', gy), ('y', y), ('post', post), ('g_z', torch.full((n, w), NAN)), ('g_res', res0), ('g_post', post0)):
                if vals is not None:
                    view, parent, ld = _place(vals, True, ACT_PITCH[name] - w)
                    assert ld == ACT_PITCH[name]
                    bufs[name] = (view, parent, ld, parent.clone())
            ptr = lambda k: _p(bufs[k][0]) if k in bufs else None
            ld = lambda k: bufs[k][2] if k in bufs else 0
            _check(L, L.r2l_train_act_backward(ptr('g_y'), ld('g_y'), ptr('y'), ld('y'), ptr('post'), ld('post'), n, w, code, scale,
                                               ptr('g_z'), ld('g_z'), ptr('g_res'), ld('g_res'), res_acc, ptr('g_post'), ld('g_post'), 0,
                                               _stream()))
            torch.cuda.synchronize()
            gz, gres, gpost = (bufs[k][0].cpu() for k in ('g_z', 'g_res', 'g_post'))
            assert torch.equal(gpost, gy)
            assert bool(((gz.double() - scale * gu64).abs() <= gamma(4) * (scale * gu64).abs()).all())
            want = gu64 + (res0.double() if res_acc else 0)
            assert bool(((gres.double() - want).abs() <= gamma(4) * (gu64.abs() + (res0.double().abs() if res_acc else 0))).all())
            for name, (view, parent, _, keep) in bufs.items():
                assert _only_the_window_changed(parent, keep, (n, w), True), name
                if name in ('g_y', 'y', 'post'):
                    assert _same_bits(parent, keep), name                     # the inputs are read only


# ---- 7. one whole step above 65,536 rays ---------------------------------------------------------------------------------------
def _rays(n, seed):
    """tests/test_train_gpu.py's rays: origins (0, 0, 4) + 0.2 N(0, 1), directions normalize(-o + 0.8 N(0, 1))"""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)
    d = -o + 0.8 * torch.randn(n, 3, generator=g)
    return o, d / d.norm(dim=-1, keepdim=True)


def _autograd(forward, sd, emb, target, dtype):
    """loss and gradients of mean((forward(sd, emb) - target)^2) under torch autograd in `dtype`"""
    prm = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    loss = ((forward(prm, emb.to(dtype)) - target.to(dtype)) ** 2).mean()
    loss.backward()
    return loss.item(), {k: v.grad.detach() for k, v in prm.items()}


def _gaps(got, ref):
    """(global relative L2 gap over all parameters, largest per-tensor relative L2 gap) from the float64 gradients"""
    num = {k: float((got[k].double().cpu() - ref[k]).norm()) for k in ref}
    den = {k: float(ref[k].norm()) for k in ref}
    glob = np.sqrt(sum(v ** 2 for v in num.values())) / np.sqrt(sum(v ** 2 for v in den.values()))
    return glob, max(num[k] / den[k] for k in ref)


def test_whole_step_above_65536_rays(pkg):
    """70,001 rays through R2LTrainer.forward_backward on a small residual network: the host side's workspace at the capped slab
    count, the loss's second round of partials and the GEMMs' empty slabs in one step.  Float64 autograd of the oracle's forward as
    the yardstick, torch fp32 autograd as the band (factor 4), as test_whole_network_gradients_small_variants."""
    from efficient_nerf_amd.train import R2LTrainer
    from oracle import r2l_oracle as O
    n, n_sample, D, W = STEP_RAYS, 4, 6, 64
    assert slab_rule(n)[0] == GW_MAX_SLABS and slab_rule(n)[2] and loss_partials(n)[1] == 2
    trial = dict(body_arch='resmlp', n_learnable=2)
    tr = R2LTrainer(n_sample=n_sample, L=3, netdepth=D, netwidth=W, use_residual=True, trial=trial, max_rays=n)
    sd = O.make_v3_2_state(4, D, W, tr.input_dim, '', 'relu', trial)
    tr.load_state_dict(sd)
    tr._ws.fill_(NAN)                                     # what a slab does not write would reach the gradient
    tr._grad.fill_(NAN)
    g = torch.Generator().manual_seed(207)
    ro, rd = _rays(n, 57)
    target, t_rand = torch.rand(n, 3, generator=g), torch.rand(n, n_sample, generator=g)
    emb = tr.embed(ro.cuda(), rd.cuda(), 1., t_rand.cuda()).cpu()
    loss = tr.forward_backward(ro.cuda(), rd.cuda(), target.cuda(), 1., t_rand.cuda()).item()
    got = tr.grads()
    fwd = lambda prm, x: O.v3_2_forward(prm, x, D, 'relu', True, trial)
    l64, g64 = _autograd(fwd, sd, emb, target, torch.float64)
    l32, g32 = _autograd(fwd, sd, emb, target, torch.float32)
    assert set(got) == set(g64) and all(torch.isfinite(v).all() for v in got.values())
    hip, t32 = _gaps(got, g64), _gaps(g32, g64)
    for q, label in ((0, 'global'), (1, 'per-tensor')):
        print(f'{n} rays: {label} relative L2 gap of the gradients from float64: HIP {hip[q]:.2e}, torch fp32 {t32[q]:.2e} '
              f'(ratio {hip[q] / t32[q]:.2f})')
    print(f'{n} rays: loss f64 {l64:.9f}: |HIP - f64| / f64 = {abs(loss - l64) / l64:.2e}, torch fp32 {abs(l32 - l64) / l64:.2e}')
    for q in (0, 1):
        assert hip[q] <= 4 * t32[q]
    assert abs(loss - l64) / l64 <= max(4 * abs(l32 - l64) / l64, 1e-7)
    assert torch.isfinite(tr._err[:n]).all()                                                # the per-ray error of all 70,001 rays


# ---- 8. NaN and infinity through the scan's backward pass and the element-wise kernels -----------------------------------------
# Torch on the CPU is the reference throughout: float32 autograd / torch.optim.Adam give the NaN, +Inf and -Inf masks an output
# must have element for element, float64 the values (the factor-4 band above).  The scan's cases are those of
# tests/nonfinite_cases.py (kinds a .. k at sample 0, 63, 64 and S - 1 of the odd rays), which tests/test_scan_special_gpu.py holds
# to what each kind says in the forward references; special_preconditions() does the same for the gradients.
_SCAN_GRADS = {}


def _special_scan_grads(n, S, kind, white, with_noise):
    """(clean, poisoned, float32 autograd's g_raw of the poisoned case, float64's), computed once"""
    from oracle import r2l_oracle as O
    key = (n, S, kind, white, with_noise)
    if key not in _SCAN_GRADS:
        ref = scan_reference(n, S, kind, white, with_noise)
        if ref is None:
            _SCAN_GRADS[key] = None
        else:
            clean, bad = ref[0], ref[1]
            args = (bad['raw'], bad['z'], bad['rd'], bad['g_rgb'], white, bad['noise'])
            _SCAN_GRADS[key] = (clean, bad, _scan_autograd(O, *args, torch.float32), _scan_autograd(O, *args, torch.float64))
    return _SCAN_GRADS[key]


def special_preconditions():
    for S in SPECIAL_S:
        for n in SPECIAL_N:
            for kind, white, with_noise in scan_combos():
                ref = _special_scan_grads(n, S, kind, white, with_noise)
                if ref is None:
                    continue
                clean, bad, g32, g64 = ref
                tag = (n, S, kind, white, with_noise)
                assert same_masks(g32, g64.float()), tag
                rays = poisoned_rays(n)
                others = [r for r in range(n) if r not in rays]
                assert torch.isfinite(g32[others]).all() and torch.isfinite(g64[others]).all(), tag
                if kind in 'abdfhjk':                               # a NaN reaches the gradient of every poisoned ray (i: disp alone is NaN) ...
                    assert all(torch.isnan(g32[r]).any() for r in rays), tag
                pre = bad['raw'][..., 3] + (bad['noise'] if bad['noise'] is not None else 0.)
                assert not g32[..., 3][pre <= 0].any(), tag             # ... and never a closed relu: threshold_backward gives 0 there
    return True


special_preconditions()


def _masked_rel(got, ref, keep):
    d, r = ((got.double() - ref.double()) ** 2)[keep], (ref.double() ** 2)[keep]
    return float(d.sum().sqrt() / r.sum().sqrt()) if float(r.sum()) > 0 else float(d.sum().sqrt())


FEW_NUMBERS = SCAN_CHUNK * 4        # one chunk of one ray: 64 samples x 4 channels


def _few_numbers(g64, gap_t32):
    """Decided from the references alone.  The factor 4 compares two averages of rounding errors; over a handful of numbers torch's
    own can be 0 or near it by luck (S = 2 on one ray is eight numbers, of which the last density's gradient is an exact 0), and the
    ratio then says nothing about the kernel.  A case is held to 4 x its own torch-fp32 gap when at least one chunk of one ray's worth
    of float64-finite, non-zero gradients remains and torch-fp32's gap is not 0; a case with fewer is held to 4 x the largest
    torch-fp32 gap over the cases of its (S, n).  With the cases of this file those are: every case of S = 2; every case of S = 17 at
    n = 1 and n = 5, and at n = 9 the kinds that make the four odd rays NaN (a, b, d, h, i, j, k); at n = 1, where the one ray is the
    poisoned one, every case of S = 64 and 65, S = 129 but for kinds e and g, and at S = 193 and 256 the kinds a, b, d, h, i, j, k
    (kinds i, j, k leave nothing finite there: both gaps are 0).  No case of n = 5 or n = 9 from S = 64 on is among them."""
    kept = int((torch.isfinite(g64) & (g64 != 0)).sum())
    return gap_t32 == 0 or kept < FEW_NUMBERS


@pytest.mark.parametrize('n', SPECIAL_N)
@pytest.mark.parametrize('S', SPECIAL_S)
def test_scan_backward_non_finite_inputs(L, S, n):
    """nerf_train_raw2outputs_backward on kinds (a) .. (k) against autograd of the oracle: g_raw has float32 autograd's NaN, +Inf and
    -Inf masks element for element -- NaN at the poisoned sample itself, an exact 0 wherever the relu is closed -- and over the
    elements that are finite in float64 its gap from float64 autograd is, case by case (kind, white, noise), at most 4 x
    torch-fp32's of that case, as in test_scan_backward_with_a_ragged_last_chunk; only the cases _few_numbers names are held to the
    largest torch-fp32 gap of their (S, n) instead.  The clean rays keep the bits of a launch without the poison; nothing is written
    beside [n, S, 4]; twice the same bits.  On an MI355X the largest ratio of a case held to its own gap is 2.0 (488 cases); of the
    394 cases of few numbers one, S = 2, n = 1, kind e, is above 4 x its own (1.27e-7 against 2.46e-8 over eight numbers).

    Kinds c, d and k (+Inf density) are held to the same rule as the others.  Autograd's cumprod backward divides by p = 1e-10 on the
    saturated sample where the kernel's B is the division-free recurrence (csrc/nerf_train.hip's header), but neither turns an
    element non-finite that the other keeps: on an MI355X no element's mask differs in any of the 21 x 42 cases."""
    gaps = []
    for kind, white, with_noise in scan_combos():
        ref = _special_scan_grads(n, S, kind, white, with_noise)
        if ref is None:
            continue
        clean, bad, g32, g64 = ref
        tag = (kind, white, with_noise)
        got, margins = _scan_hip(L, bad['raw'], bad['z'], bad['rd'], bad['g_rgb'], white, bad['noise'])
        again, _ = _scan_hip(L, bad['raw'], bad['z'], bad['rd'], bad['g_rgb'], white, bad['noise'])
        base, _ = _scan_hip(L, clean['raw'], clean['z'], clean['rd'], clean['g_rgb'], white, clean['noise'])
        rays = poisoned_rays(n)
        others = [r for r in range(n) if r not in rays]
        assert torch.isnan(margins).all(), tag
        assert same_bits(got, again), tag
        if others:
            assert same_bits(got[others], base[others]) and torch.isfinite(got[others]).all(), tag
        pre = bad['raw'][..., 3] + (bad['noise'] if bad['noise'] is not None else 0.)
        assert not got[..., 3][pre <= 0].any(), tag                         # exactly 0 where the relu is closed
        assert same_masks(got, g32), tag
        keep = torch.isfinite(g64)
        gap_hip, gap_t32 = _masked_rel(got, g64, keep), _masked_rel(g32, g64, keep)
        few = _few_numbers(g64, gap_t32)
        print(f'S={S} n={n} {kind} white={white} noise={with_noise}: relative L2 gap from float64: HIP {gap_hip:.2e}, torch fp32 {gap_t32:.2e}'
              f'{" (few numbers: pooled)" if few else ""}')
        if not few:
            assert gap_hip <= 4 * gap_t32, (tag, gap_hip, gap_t32)                # the file's rule, case by case
        gaps.append((gap_hip, gap_t32, tag, few))
    # the cases of few numbers against the largest torch-fp32 gap of this (S, n), as _band_check of tests/test_train_gpu.py pools
    band = max(r[1] for r in gaps)
    for gap_hip, gap_t32, tag, few in gaps:
        if few:
            assert gap_hip <= 4 * band, (tag, gap_hip, band)


ACT_U = [NAN, INF, -INF, 1.5, -1.5, 0.]
ACT_GY = [NAN, INF, -INF, 0.75, -0.75, 0.]


def _act_special_case(act, seed):
    """v, res, post, g_y [37, 9]: the activation's input u = s v + res takes each of ACT_U against each of ACT_GY (36 elements
    among 333), everything else finite with |u| >= 0.5 (so that y - post keeps u's sign); post finite"""
    g = torch.Generator().manual_seed(seed)
    n, w, s = 37, 9, 0.5
    sign = torch.where(torch.rand(n, w, generator=g) < 0.5, -1., 1.)
    u = sign * (0.5 + torch.rand(n, w, generator=g))
    gy = torch.randn(n, w, generator=g)
    where = torch.randperm(n * w, generator=g)[:36]
    for k, idx in enumerate(where.tolist()):
        u.view(-1)[idx], gy.view(-1)[idx] = ACT_U[k // 6], ACT_GY[k % 6]
    res = torch.randn(n, w, generator=g) * 0.25
    v = (u - res) / s                                   # s v + res reproduces u's specials (and the finite values to an ulp)
    post = torch.rand(n, w, generator=g) - 0.5
    return v, res, post, gy, s, where


def _act_torch(act, v, res, post, gy, s, dtype):
    fn = {'none': lambda x: x, 'relu': torch.relu, 'lrelu': torch.nn.functional.leaky_relu, 'sigmoid': torch.sigmoid}[act]
    leaf = [t.to(dtype).clone().requires_grad_(True) for t in (v, res)] + ([post.to(dtype).clone().requires_grad_(True)] if post is not None else [])
    y = fn(s * leaf[0] + leaf[1])
    if post is not None:
        y = leaf[2] + y
    y.backward(gy.to(dtype))
    return y.detach(), [t.grad for t in leaf]


@pytest.mark.parametrize('act', ['none', 'relu', 'lrelu', 'sigmoid'])
def test_act_backward_non_finite_against_autograd(L, act):
    """r2l_train_act_backward against torch autograd of y = post + act(s v + res) per element (not the restated y - post formula):
    NaN, +Inf and -Inf in the activation and in g_y, g_res and g_post overwritten and accumulated.  g_z (= g_v), g_res and g_post
    have float32 autograd's masks; their finite elements are within the factor-4 band of float64 autograd.  relu at a NaN
    activation passes g_y, at a closed one gives 0 whatever g_y holds (threshold_backward); lrelu multiplies.  post stays finite:
    the kernel recovers the activation as y - post, and an infinite post makes that NaN by construction."""
    code = {'none': 0, 'relu': 1, 'lrelu': 2, 'sigmoid': 3}[act]
    v, res, post, gy, s, where = _act_special_case(act, 60 + code)
    n, w = v.shape
    for with_post in (False, True):                     # sigmoid too, though the trainers never give it a skip
        pst = post if with_post else None
        y32, g32 = _act_torch(act, v, res, pst, gy, s, torch.float32)
        _, g64 = _act_torch(act, v, res, pst, gy, s, torch.float64)
        assert all(same_masks(a, b.float()) for a, b in zip(g32, g64))                   # the precondition, on the CPU
        assert not torch.isfinite(g32[0].view(-1)[where]).all() and torch.isfinite(g32[0]).any()
        g = torch.Generator().manual_seed(61)
        res0, post0 = torch.randn(n, w, generator=g), torch.randn(n, w, generator=g)
        for acc in (0, 1):
            d = {k: t.cuda().contiguous() for k, t in (('g_y', gy), ('y', y32), ('g_res', res0), ('g_post', post0))}
            d['g_z'] = torch.full((n, w), NAN, device='cuda')
            pd = pst.cuda().contiguous() if with_post else None
            _check(L, L.r2l_train_act_backward(_p(d['g_y']), w, _p(d['y']), w, _p(pd), w if with_post else 0, n, w, code, s, _p(d['g_z']), w,
                                               _p(d['g_res']), w, acc, _p(d['g_post']) if with_post else None, w if with_post else 0, acc,
                                               _stream()))
            torch.cuda.synchronize()
            want32 = [g32[0], g32[1] + (res0 if acc else 0)] + ([g32[2] + (post0 if acc else 0)] if with_post else [])
            want64 = [g64[0], g64[1] + (res0.double() if acc else 0)] + ([g64[2] + (post0.double() if acc else 0)] if with_post else [])
            for name, a32, a64 in zip(('g_z', 'g_res', 'g_post'), want32, want64):
                got = d[name].cpu()
                assert same_masks(got, a32), (act, with_post, acc, name)
                keep = torch.isfinite(a64) & torch.isfinite(a32)
                gap_hip, gap_t32 = _masked_rel(got, a64, keep), _masked_rel(a32, a64, keep)
                print(f'{act} post={with_post} acc={acc} {name}: relative L2 gap from float64: HIP {gap_hip:.2e}, torch fp32 {gap_t32:.2e}')
                assert gap_hip <= 4 * gap_t32, (act, with_post, acc, name, gap_hip, gap_t32)
            if not with_post:
                assert _same_bits(d['g_post'].cpu(), post0)                                 # not asked for: not written


MSE_N = 513
MSE_RAYS = [0, 255, 256, MSE_N - 1]


def _mse_torch(rgb, tgt, through, dtype):
    r = rgb.to(dtype).clone().requires_grad_(True)
    d2 = (r - tgt.to(dtype)) ** 2
    loss = d2.mean()
    loss.backward()
    g = torch.ops.aten.sigmoid_backward(r.grad, r.detach()) if through else r.grad      # torch's own sigmoid backward at the output rgb
    return loss.detach(), g, d2.detach().mean(1)


@pytest.mark.parametrize('through', [0, 1])
@pytest.mark.parametrize('ray', MSE_RAYS)
def test_mse_loss_with_one_non_finite_ray(L, ray, through):
    """513 rays, a NaN or an infinity in one channel of rgb or of the target of ray 0, 255, 256 (either side of the partial sums'
    block edge) or 512: the loss is NaN or Inf as torch's, g_out and the per-ray error have torch-float32's masks (non-finite on
    that ray alone, in the channels torch says), and every other ray keeps the bits of the clean launch"""
    g = torch.Generator().manual_seed(90 + ray + through)
    n = MSE_N
    rgb, tgt = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    base = _mse(L, rgb.cuda(), tgt.cuda(), n, through)
    others = [r for r in range(n) if r != ray]
    for value, where in ((NAN, 'rgb'), (INF, 'target'), (NAN, 'target'), (-INF, 'rgb'), (INF, 'rgb')):
        r2, t2 = rgb.clone(), tgt.clone()
        (r2 if where == 'rgb' else t2)[ray, 1] = value
        l32, g32, e32 = _mse_torch(r2, t2, through, torch.float32)
        l64, g64, e64 = _mse_torch(r2, t2, through, torch.float64)
        assert same_masks(g32, g64.float()) and same_masks(e32, e64.float()) and same_masks(l32, l64.float())
        assert not torch.isfinite(l32) and not torch.isfinite(e32[ray]) and torch.isfinite(e32[others]).all()
        loss, gout, err = _mse(L, r2.cuda(), t2.cuda(), n, through, finite=False)
        loss2, gout2, err2 = _mse(L, r2.cuda(), t2.cuda(), n, through, finite=False)
        tag = (ray, through, value, where)
        assert same_masks(loss.cpu().view(()), l32), tag
        assert same_masks(gout.cpu(), g32), tag
        assert same_masks(err.cpu(), e32), tag
        assert _same_bits(gout[others], base[1][others]) and _same_bits(err[others], base[2][others]), tag
        assert same_bits(gout.cpu(), gout2.cpu()) and same_bits(err.cpu(), err2.cpu()) and same_bits(loss.cpu(), loss2.cpu()), tag


ADAM_COUNT = 257
ADAM_SPECIAL = {3: NAN, 128: INF, 200: -INF, 254: 0., 255: 1e-30, 256: 3e38}         # on both sides of the edge at 256
# gradients that change from step to step: a finite one behind an infinite one (exp_avg = inf + (1 - b1) (g - inf) = NaN in torch's
# lerp_, where m b1 + (1 - b1) g keeps inf), and one whose g - m overflows (lerp_: -inf, then NaN; the products stay finite)
ADAM_SEQUENCES = {130: (INF, 0.5, -0.5), 131: (3.4e38, -3.4e38, 3.4e38)}


def _torch_adam_state(p0, grads, lr, dtype):
    prm = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adam([prm], lr=lr, betas=(0.9, 0.999))
    for gr in grads:
        prm.grad = gr.to(dtype).clone()
        opt.step()
    st = opt.state[prm]
    return prm.detach(), st['exp_avg'].detach(), st['exp_avg_sq'].detach()


def _hip_adam(L, p0, grads, lr):
    (pb, p), (mb, m), (vb, v), (gb, gr_d) = (_margined(p0.numel()) for _ in range(4))
    p.copy_(p0)
    m.zero_()
    v.zero_()
    for k, gr in enumerate(grads):
        gr_d.copy_(gr)
        _check(L, L.r2l_train_adam(_p(p), _p(gr_d), _p(m), _p(v), p0.numel(), lr, k + 1, _stream()))
    torch.cuda.synchronize()
    assert all(_margins_are_nan(b, p0.numel()) for b in (pb, mb, vb, gb))
    return p.cpu(), m.cpu(), v.cpu()


def test_adam_with_non_finite_and_extreme_gradients(L):
    """257 elements, 3 steps; one element each whose gradient is NaN, +Inf, -Inf (p = NaN: inf / inf), 0 on zero state, 1e-30 (g^2
    underflows: v = 0 and p moves by lr m^ / eps) and 3e38 (g^2 overflows: v = inf and p stays), on both sides of the block edge.  p,
    m and v have float32 torch.optim.Adam's masks.  The ordinary elements are within 4 x torch-fp32's largest gap from float64
    Adam; a special element, whose float32 result is by design far from float64's (v = inf against 9e76), within 4 x the larger of
    that band and torch-fp32's own gap at that element.  The ordinary elements keep the bits of a run without the special ones.

    That band says little at 3e38, so a special element that stays finite is also held to float32 torch.optim.Adam itself, within
    gamma(32): over the three steps each side rounds at most 16 times on the way to it (per step the coefficient and three
    operations of m carried forward, then multiply, divide, add for p), all on values of one sign, so nothing cancels.  The 1e-30
    element starts at p = 0, where its steps of 1e-25 show.  Two more elements change their gradient from step to step
    (ADAM_SEQUENCES): m is NaN there as torch's lerp_ makes it."""
    g = torch.Generator().manual_seed(17)
    count, lr = ADAM_COUNT, 1e-3
    p0 = torch.randn(count, generator=g)
    p0[255] = 0.
    plain = [torch.randn(count, generator=g) * 10 ** (-6 * torch.rand(count, generator=g)) for _ in range(3)]
    grads = [t.clone() for t in plain]
    for k, t in enumerate(grads):
        for idx, val in ADAM_SPECIAL.items():
            t[idx] = val
        for idx, vals in ADAM_SEQUENCES.items():
            t[idx] = vals[k]
    ref32, ref64 = _torch_adam_state(p0, grads, lr, torch.float32), _torch_adam_state(p0, grads, lr, torch.float64)
    assert torch.isnan(ref32[0][[3, 128, 200]]).all() and torch.isinf(ref32[2][256]) and ref32[2][255] == 0     # what the elements are for
    assert ref32[0][255] != 0 and torch.isnan(ref32[1][[130, 131]]).all() and torch.isfinite(ref64[1][131])
    got, got2, base = _hip_adam(L, p0, grads, lr), _hip_adam(L, p0, grads, lr), _hip_adam(L, p0, plain, lr)
    ordinary = torch.ones(count, dtype=torch.bool)
    ordinary[list(ADAM_SPECIAL) + list(ADAM_SEQUENCES)] = False
    for name, a, a2, b, r32, r64 in zip('pmv', got, got2, base, ref32, ref64):
        assert same_masks(a, r32), name
        assert same_bits(a, a2), name
        assert _same_bits(a[ordinary], b[ordinary]), name
        gap_hip, gap_t32 = (a.double() - r64).abs(), (r32.double() - r64).abs()
        band = float(gap_t32[ordinary].max())
        print(f'Adam {name}: ordinary elements max gap HIP {float(gap_hip[ordinary].max()):.3e}, torch fp32 {band:.3e}')
        assert float(gap_hip[ordinary].max()) <= 4 * band, name
        for idx in list(ADAM_SPECIAL) + list(ADAM_SEQUENCES):
            if torch.isfinite(r32[idx]) and torch.isfinite(r64[idx]):
                assert float(gap_hip[idx]) <= 4 * max(band, float(gap_t32[idx])), (name, idx)
            if torch.isfinite(r32[idx]):
                off = abs(float(a[idx]) - float(r32[idx]))
                print(f'Adam {name}[{idx}]: HIP {float(a[idx])!r}, torch fp32 {float(r32[idx])!r}')
                assert off <= gamma(32) * abs(float(r32[idx])), (name, idx, float(a[idx]), float(r32[idx]))

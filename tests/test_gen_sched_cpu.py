"""The machinery the three stream generators share (csrc/gen/isa.py): the list scheduler on a toy, the tracker of the
counted lgkmcnt waits, the option sets, and that none of it keeps state between two generators or two runs of one."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'efficient-nerf_amd', 'csrc', 'gen'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa  # noqa: E402
import body_gen  # noqa: E402
import head_gen  # noqa: E402
import test_nerf_genx_cpu as TX  # noqa: E402  (INST: one instance of nerf_gen per variant)

N_ANCHORS = 12


def _valu(name):
    return isa.Ins(name, 'valu')


def _toy():
    """three chains; returns {name: (earliest, deadline)} as written and the fillers in the order a generator would build them"""
    win = {'A0': (-1, 2), 'A1': (0, 9), 'A2': (1, 4), 'A3': (5, 8), 'A4': (6, 12)}     # A1's deadline is later than its successor's
    win.update({'B%d' % i: (0, 6) for i in range(10)})                                   # ten fillers that want the slots A1 needs
    win.update({'C0': (3, 11), 'C1': (20, 50)})                                          # C1 may not issue behind any anchor
    return win, [isa.Filler(_valu(n), e, d, (n[0],)) for n, (e, d) in win.items()]


def _run(F, budget):
    sch = isa.Sched()
    ls = isa.ListSched(F, sch)
    ls.start()
    for a in range(N_ANCHORS):
        ls.due(a)
        sch.emit(isa.Ins('anchor', 'mfma16', tag=a))
        ls.fill(a, budget)
    ls.finish()
    return sch.out


def test_list_scheduler_on_a_toy():
    win, F = _toy()
    out = _run(F, 2)
    last = {}                      # filler -> the last anchor emitted in front of it (-1: none)
    a = -1
    for ins in out:
        if ins.kind == 'mfma16':
            a = ins.tag
        else:
            last[ins.text] = a
    assert sorted(last) == sorted(win) and len(out) == len(win) + N_ANCHORS          # everything issued, once
    order = [ins.text for ins in out if ins.kind != 'mfma16']
    for ch in 'ABC':               # fillers of a chain keep their order
        assert [n for n in order if n[0] == ch] == [n for n in win if n[0] == ch]
    for n, (e, d) in win.items():
        if n == 'C1':
            continue
        assert e <= last[n] < d, (n, e, last[n], d)          # behind anchor `earliest`, in front of anchor `deadline`
    # A1 alone (deadline 9) loses every slot to the B fillers (deadline 6) and would hold A2 back past anchor 4
    assert last['A1'] <= last['A2'] < 4
    # what is left drains at the end
    assert last['C1'] == N_ANCHORS - 1 and order[-1] == 'C1'


def test_budget_is_charged_in_issue_slots():
    def behind_anchor_0(make):
        F = [isa.Filler(make(i), 0, 100, ('x',)) for i in range(8)]
        out = _run(F, 6)
        i0 = next(i for i, ins in enumerate(out) if ins.kind == 'mfma16')
        i1 = next(i for i, ins in enumerate(out) if ins.kind == 'mfma16' and ins.tag == 1)
        return i1 - i0 - 1
    assert isa.s_nop(3).cost == 4 and _valu('v').cost == 1
    assert behind_anchor_0(lambda i: _valu('v%d' % i)) == 6
    assert behind_anchor_0(lambda i: isa.s_nop(3)) == 2          # 6 - 4 = 2 slots left: one more, then the budget is spent


def _read(tag):
    return isa.Ins('ds_read %s' % (tag,), 'ds', tag=tag)


def test_tracker_clamps_the_wait_to_the_four_bit_counter():
    sch = isa.Sched()
    for i in range(20):
        sch.emit(_read(('r', i)))
    sch.need(('r', 0))
    assert sch.out[-1].text == 's_waitcnt lgkmcnt(15)' and len(sch.out) == 21
    assert sch.ds_issued - sch.ds_done == 15          # 15 reads may still be out, not 19: reads 0..4 have landed
    sch.need(('r', 4))                                # covered: nothing emitted
    assert len(sch.out) == 21
    sch.need(('r', 5))
    assert sch.out[-1].text == 's_waitcnt lgkmcnt(14)' and sch.ds_done == 6


def test_tracker_also_keys_ride_along_once_issued():
    sch = isa.Sched()
    for i in range(3):
        sch.emit(_read(('r', i)))
    sch.need(('r', 0), also=[('r', 1), ('late',)])    # ('late',) is not issued yet: ignored
    assert sch.out[-1].text == 's_waitcnt lgkmcnt(1)' and sch.ds_done == 2
    sch.emit(_read(('late',)))
    n = len(sch.out)
    sch.need(('r', 1))                                # rode along
    assert len(sch.out) == n
    sch.need(('r', 2), also=[('late',)])
    assert sch.out[-1].text == 's_waitcnt lgkmcnt(0)' and sch.ds_done == sch.ds_issued == 4


def test_tracker_iteration_zero_and_landed():
    sch = isa.Sched()
    with pytest.raises(KeyError):
        sch.need(('never',))
    sch.it = 0                                         # a read of the iteration before the schedule starts
    sch.need(('never',))
    assert sch.out == []
    sch.it = 1
    with pytest.raises(KeyError):
        sch.need(('never',))
    sch.emit(_read(('r', 0)))
    sch.emit(isa.waitcnt_lgkm(0))
    sch.landed()
    sch.need(('r', 0))
    assert len(sch.out) == 2 and sch.its == [1, 1]


def _texts(stream):
    return [ins.text for ins in stream]


def test_no_state_leaks_between_generators():
    A, B = TX.INST['bf6'], TX.INST['f16c4']
    a0 = _texts(A.block_stream(A.Opts()))
    b0 = _texts(B.block_stream(B.Opts()))
    assert a0 != b0 and _texts(A.block_stream(A.Opts())) == a0
    h0 = _texts(head_gen.block_stream(head_gen.Opts(fmt='bf6')))
    hx = _texts(head_gen.block_stream(head_gen.Opts(fmt='f16')))
    assert h0 != hx and _texts(head_gen.block_stream(head_gen.Opts(fmt='bf6'))) == h0
    s0 = [_texts(x) for x in body_gen.steady_block(body_gen.Opts(fmt='bf6'))]
    s8 = [_texts(x) for x in body_gen.steady_block(body_gen.Opts(fmt='fp8'))]
    assert s0 != s8 and [_texts(x) for x in body_gen.steady_block(body_gen.Opts(fmt='bf6'))] == s0


@pytest.mark.parametrize('G, used', [
    (body_gen, dict(dma_burst=True, rd_lead=4, rd_lead6=4, cap16=6, cap6=6, dma_gap=None, chain_nop=-1, guard=True, fmt='fp8', stage=False,
                    shallow_ring=False, rdv_at=None, wait_group=None, wait_group6=None, skip_terms=(0,), drop=('lgkm',))),
    (head_gen, dict(rd_lead=6, rd_lead6=5, cap=7, dma_gap=1, pair_waits=False, fmt='f16')),
    (TX.INST['bf6'], dict(pair=True, drop=('dma',), lead=8, lead6=5, cap=3, dma_gap=4, wait_group=2)),
], ids=['body', 'head', 'chain'])
def test_options_are_declared(G, used):
    with pytest.raises(TypeError, match='rd_laed'):
        G.Opts(rd_laed=3)
    o = G.Opts(**used)             # every keyword a main(), a tool script or a test passes
    assert all(getattr(o, k) == v for k, v in used.items())
    assert G.Opts().drop == ()

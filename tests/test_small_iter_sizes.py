"""The windows of tests/test_small_iter_sizes_gpu.py, checked on the CPU: (1) from WindowBuilder and the constants of
csrc/small.hip alone, every case lands on the side of every size switch it is there for -- retuning a constant fails here instead
of silently losing the coverage; (2) the fp64 yardstick with the bounds of the GPU test notices single faults of the kind a wrong
tile bound, CSR run or slab index would make."""
import pytest
import torch

from oracle import trackmpnn_oracle as orc
from tests import small_iter_cases as sc


@pytest.fixture(scope='module')
def K():
    return sc.kernel_constants()


def _calls(case):
    return sc.window_calls(sc.FRAMES[case])


def test_constants_are_the_ones_the_cases_were_sized_for(K):
    """The two BatchNorm-backward row limits are one number written twice; the python binding restates the header."""
    from trackmpnn_amd.graph import DG_MAX_ROWS
    assert K['BN_LDS_ROWS'] == K['BN_LDS_ROWS_C']
    assert K['DG_MAX_ROWS'] == DG_MAX_ROWS
    assert K['DET_TILE_SMALL'] < K['TR']


def test_case_a_loops_over_several_tiles_per_backward_block(K):
    c0, c1, c2 = _calls('A')
    assert [c.N for c in (c0, c1, c2)] == [624, 1224, 1824]
    TR = K['TR']
    for c, capped in ((c0, False), (c1, False), (c2, True)):
        nEt, nDt = -(-c.E // TR), -(-c.Dn // TR)
        nb = sc.bwd_blocks(c.N, K)
        assert (nb == K['SMALL_BWD_BLOCKS'] and nEt + nDt > nb) == capped, (c.N, nEt, nDt, nb)
        if capped:
            nbE = sc.bwd_edge_blocks(nEt, nDt, nb)
            assert nEt > nbE and nDt > nb - nbE, 'both cells must have a block with more than one tile'
            assert nEt + nDt == 114
    # the first calls stay below the cap: one launch of the window takes the one-tile form, one the looping form
    assert c0.N <= (K['SMALL_BWD_BLOCKS'] - 2) * TR < c2.N


def test_case_b_has_more_new_dets_than_the_lds_holds_on_four_det_tiles(K):
    c0, c1 = _calls('B')
    assert (c0.N, c0.E, c0.nd) == (3843, 3721, 122) and c1.N == 4091
    assert c0.nd > K['BN_LDS_ROWS'] and c0.nd > K['BN_LDS_ROWS_C']
    assert c0.nd > K['CH'], 'the input transform walks a second chunk'
    assert c0.N <= K['DG_MAX_ROWS'] and c1.N <= K['DG_MAX_ROWS'], 'det_tile = 4 in both calls'
    assert c1.N - c1.n_new == 3843 and 0 < c1.nd <= K['BN_LDS_ROWS']
    assert c0.tile_incidences(K['DET_TILE_SMALL']).max() <= K['SINC'], 'the staged form of the 4-det tile'


def test_case_c_runs_sixteen_det_tiles_unstaged_and_grid_strides_the_carried_rows(K):
    """(The carried-row adjoint grid-strides beyond ROW_BLOCKS * 1024 / H rows: 4096 at H = 64, 8192 at H = 32.  Case C carries
    5040 rows, so that route is reached by its H = 64 models only; every other condition holds at both widths.)"""
    c0, c1 = _calls('C')
    assert (c0.N, c0.nd) == (5040, 140) and c1.N == 5466
    assert c0.N > K['DG_MAX_ROWS'] and c1.N > K['DG_MAX_ROWS'], 'det_tile = TR in both calls'
    inc0 = c0.tile_incidences(K['TR'])
    assert inc0.max() == 1120 and inc0.max() > K['SINC'], 'a 16-det tile longer than the staged stretch'
    inc1 = c1.tile_incidences(K['TR'])
    assert inc1.max() > K['SINC'] and inc1.min() <= K['SINC'], 'the second call has both forms in one launch'
    assert c0.nd > K['BN_LDS_ROWS'] and c0.nd > K['BN_LDS_ROWS_C'] and c0.nd > 2 * K['CH']
    assert 0 < c1.nd <= K['BN_LDS_ROWS'], 'new det rows on both sides of the LDS limit (a wide feature group is unstaged on both)'
    n_old = c1.N - c1.n_new
    H = 64
    assert n_old == 5040 and n_old > K['ROW_BLOCKS'] * (1024 // H), 'the carried-row adjoint grid-strides at H = 64'
    assert n_old > K['DG_MAX_ROWS']
    assert n_old <= K['ROW_BLOCKS'] * (1024 // 32), 'stated above: not at H = 32'
    for c in (c0, c1):
        TR = K['TR']
        assert -(-c.E // TR) + -(-c.Dn // TR) > 3 * K['SMALL_BWD_BLOCKS'], 'every backward block loops'


def test_case_d_runs_four_det_tiles_unstaged(K):
    c0, c1 = _calls('D')
    assert (c0.N, c0.nd) == (3200, 300) and c1.N == 4073
    assert c0.N <= K['DG_MAX_ROWS'] and c1.N <= K['DG_MAX_ROWS'], 'det_tile = 4 in both calls'
    assert int(c0.degrees().max()) == 290
    inc = c0.tile_incidences(K['DET_TILE_SMALL'])
    assert inc.max() == 1160 and inc.max() > K['SINC'], '4-det tiles of the first frame: longer than the staged stretch'
    assert inc.min() <= K['SINC'], 'the later frame takes the staged form in the same launch'
    assert c0.nd > K['BN_LDS_ROWS'] and c0.nd > K['BN_LDS_ROWS_C'] and c0.nd > 4 * K['CH']
    assert 0 < c1.nd <= K['BN_LDS_ROWS']


def test_case_e_has_exactly_full_tiles_and_less_than_one_tile(K):
    TR, TD = K['TR'], K['DET_TILE_SMALL']
    full = _calls('E4')
    assert len(full) == 2
    for c in full:
        assert c.E > 0 and c.E % TR == 0 and c.Dn % TD == 0, (c.E, c.Dn)
    short = _calls('E3')
    assert (short[0].E, short[0].Dn) == (2, 3)
    assert short[0].E < TR and short[0].Dn < TD and short[0].N < TR
    assert all(c.E % TR != 0 and c.Dn % TD != 0 for c in short)


# ------------------------------------------------------------------------------------------------------------
# would the comparison of the GPU test notice?  fp64 oracle only
# ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['C', 'D'])
def window(request):
    case = request.param
    cfg = orc.OracleConfig('2d', sc.NCAT, 64, 0, 'diff')
    seed = sc.SEEDS.get((case, '2d', 64, 'diff'), 0)
    params = orc.random_params(cfg, seed=seed, scale=sc.PARAM_SCALE)
    calls, xs, weights, V = sc.inputs(case, cfg, seed)
    r64 = sc.run_oracle(cfg, params, calls, xs, weights, V, torch.float64)
    r32 = sc.run_oracle(cfg, params, calls, xs, weights, V, torch.float32)
    return cfg, params, calls, xs, weights, V, r32, r64


def _moved(faulted, r32, r64):
    """the largest movement of a compared quantity in units of the bound the GPU test holds that quantity to on this window
    (2 x the fp32 oracle's own distance from fp64 + the floor)"""
    cmp = sc.compare(faulted, r32, r64)
    return max((e / b, k) for k, (e, b, _o) in cmp.items() if b > 0)


def test_one_src_off_by_one_det_is_noticed(window):
    cfg, params, calls, xs, weights, V, r32, r64 = window
    bad = sc.run_oracle(cfg, params, calls, xs, weights, V, torch.float64, graphs=sc.graphs_with_one_src_moved(calls))
    ratio, what = _moved(bad, r32, r64)
    assert ratio >= 10.0, (ratio, what)


def test_one_incidence_dropped_from_a_segment_sum_is_noticed(window):
    cfg, params, calls, xs, weights, V, r32, r64 = window
    bad = sc.run_oracle(cfg, params, calls, xs, weights, V, torch.float64, factor_gru=sc.factor_gru_dropping_last_incidence(cfg))
    ratio, what = _moved(bad, r32, r64)
    assert ratio >= 10.0, (ratio, what)


def test_one_tile_missing_from_a_gradient_slab_is_noticed(window):
    cfg, params, calls, xs, weights, V, r32, r64 = window
    bad = sc.run_oracle(cfg, params, calls, xs, sc.weights_without_last_edge_tile(calls, weights), V, torch.float64)
    for a, b in zip(bad.outs, r64.outs):
        assert torch.equal(a[2], b[2]), 'the forward does not read the loss weights'
    ratio, what = _moved(bad, r32, r64)
    assert what[0] in ('grad', 'x.grad') and ratio >= 10.0, (ratio, what)


def test_the_restated_step_equals_the_oracle_step(window):
    """The faulted message-passing step restates the oracle's: without its fault it must be the same function."""
    cfg, params, calls, xs, weights, V, r32, r64 = window
    step = sc.factor_gru_dropping_last_incidence(cfg, drop=False)
    same = sc.run_oracle(cfg, params, calls, xs, weights, V, torch.float64, factor_gru=step)
    for a, b in zip(same.outs, r64.outs):
        assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
    for k, v in r64.grads.items():
        assert torch.equal(same.grads[k], v), k

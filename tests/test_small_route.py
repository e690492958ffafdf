"""plan_small_route: what one batch-1 call runs (fused or staged, true or padded width, native or Python node, how the
parameter gradients travel), decided once from host values.  No launch, no GPU: CPU models supply the model facts, and the
table is held against a literal copy of the if / elif ladders TrackMPNN.forward_dgraph and its padded twin used to carry."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from trackmpnn_amd import TrackMPNN, loops
from trackmpnn_amd import small as S
from trackmpnn_amd.graph import DG_BIG_ROWS
from trackmpnn_amd.small import SmallRoute, plan_small_route, small_eligible

MODELS = {'h64': (64, 0), 'h48': (48, 0), 'h64k2': (64, 2), 'h128': (128, 0)}


def _facts(key):
    H, K = MODELS[key]
    m = TrackMPNN('2d', 3, H, K, 'diff')
    return m, (m._small.eligible, m._small.att, m._padded)


def _route(key, N=100, cap=None, grad_on=True, x_grad=False, h_grad=False, any_pg=True, all_pg=True, inplace=False, native=True):
    return plan_small_route(*_facts(key)[1], N, N if cap is None else cap, grad_on, x_grad, h_grad, any_pg, all_pg, inplace, native)


def test_model_facts():
    assert _facts('h64')[1] == (True, False, False)
    assert _facts('h48')[1] == (True, False, True)
    assert _facts('h64k2')[1] == (True, True, False)
    assert _facts('h128')[1] == (False, False, False)


def test_path():
    for key in ('h64', 'h48', 'h64k2'):
        assert _route(key).path == 'fused' and _route(key).padded == (key == 'h48')
        assert [_route(key, N=N).path for N in (0, 1, 65535, 65536)] == ['staged', 'fused', 'fused', 'staged']
    assert DG_BIG_ROWS == 65535
    assert [_route('h128', N=N).path for N in (0, 1, 65535, 65536)] == ['staged'] * 4
    assert plan_small_route(True, True, True, 100, 100, True, False, False, True, True, False, True).path == 'staged'   # padded with heads
    r = _route('h128', x_grad=True, any_pg=False, all_pg=False)
    assert r == SmallRoute('staged', False, '', '', True) and not _route('h128', grad_on=False).need_grad


def test_native_width():
    assert _route('h64', inplace=True) == SmallRoute('fused', False, 'native', 'inplace', True)
    assert _route('h64', inplace=True, cap=101) == SmallRoute('fused', False, 'python', 'inplace', True)
    assert _route('h64', inplace=True, native=False) == SmallRoute('fused', False, 'python', 'inplace', True)
    assert _route('h64') == SmallRoute('fused', False, 'native', 'sink', True)
    assert _route('h64', cap=101) == SmallRoute('fused', False, 'python', 'autograd', True)
    assert _route('h64', native=False) == SmallRoute('fused', False, 'python', 'autograd', True)
    # a partly frozen model gets no sink: the Python node, the parameters as autograd inputs
    assert _route('h64', all_pg=False) == SmallRoute('fused', False, 'python', 'autograd', True)
    # nothing needs a gradient: the native node under no_grad -- grad mode off, or a frozen model in grad mode
    assert _route('h64', grad_on=False) == SmallRoute('fused', False, 'native', 'none', False)
    assert _route('h64', any_pg=False, all_pg=False) == SmallRoute('fused', False, 'native', 'none', False)
    assert _route('h64', grad_on=False, cap=101) == SmallRoute('fused', False, 'python', 'none', False)
    assert _route('h64', grad_on=False, native=False) == SmallRoute('fused', False, 'python', 'none', False)
    # a frozen model in grad mode whose x (or carried state) requires grad: the Python node returns the input gradients
    for kw in (dict(x_grad=True), dict(h_grad=True)):
        assert _route('h64', any_pg=False, all_pg=False, **kw) == SmallRoute('fused', False, 'python', 'autograd', True)
    # in-place accumulation is for parameter gradients: none wanted, none taken
    assert _route('h64', grad_on=False, inplace=True).grads == 'none'
    assert _route('h64', any_pg=False, all_pg=False, inplace=True, x_grad=True).grads == 'autograd'


def test_padded_width():
    assert _route('h48') == SmallRoute('fused', True, 'native', 'sink', True)
    assert _route('h48', inplace=True) == _route('h48')                      # in-place asked for on a padded width: ignored
    assert _route('h48', inplace=True, all_pg=False) == SmallRoute('fused', True, 'python', 'autograd', True)
    assert _route('h48', cap=101) == SmallRoute('fused', True, 'python', 'autograd', True)
    assert _route('h48', native=False) == SmallRoute('fused', True, 'python', 'autograd', True)
    assert _route('h48', grad_on=False) == SmallRoute('fused', True, 'native', 'none', False)
    assert _route('h48', grad_on=False, native=False) == SmallRoute('fused', True, 'python', 'none', False)
    assert _route('h48', any_pg=False, all_pg=False, x_grad=True) == SmallRoute('fused', True, 'python', 'autograd', True)


def test_attention_heads_take_the_python_node():
    assert _route('h64k2') == SmallRoute('fused', False, 'python', 'autograd', True)
    assert _route('h64k2', inplace=True) == SmallRoute('fused', False, 'python', 'inplace', True)
    assert _route('h64k2', grad_on=False) == SmallRoute('fused', False, 'python', 'none', False)
    assert _route('h64k2', any_pg=False, all_pg=False) == SmallRoute('fused', False, 'python', 'none', False)


def test_one_eligibility_answer():
    for key in MODELS:
        m, facts = _facts(key)
        for N in (0, 1, 300, 65535, 65536):
            for flags in itertools.product((False, True), repeat=7):
                assert small_eligible(m, N) == (plan_small_route(*facts, N, N, *flags).path == 'fused'), (key, N, flags)
    padded_heads = TrackMPNN('2d', 3, 48, 2, 'diff')
    assert padded_heads._small.eligible and not small_eligible(padded_heads, 100)


@pytest.mark.parametrize('native', [True, False])
def test_fast_greedy_condition_is_a_route(monkeypatch, native):
    """loops._fast_greedy hands the greedy timestep to the native driver exactly where a one-row call with grad mode off
    routes to the fused path's native node on a true width."""
    stub = SimpleNamespace(greedy_run=None) if native else None
    monkeypatch.setattr(S, 'fast_module', lambda: stub)
    for key in list(MODELS) + ['h32']:
        H, K = MODELS.get(key, (32, 0))
        m = TrackMPNN('2d', 3, H, K, 'diff').eval()
        sp = m._small
        r = plan_small_route(sp.eligible, sp.att, m._padded, 1, 1, False, False, False, False, False, False, native)
        want = (r.path, r.node, r.grads, r.padded) == ('fused', 'native', 'none', False)
        assert want == (native and key in ('h64', 'h32'))
        assert want == (not m._padded and sp.eligible and not sp.att and 0 < 1 <= DG_BIG_ROWS and native)   # as it was written
        got = loops._fast_greedy(m, False, True, None)
        assert (got[0] is not None) == want and got[2] == 0 and (got[0] is stub or not want)
        assert loops._fast_greedy(m, False, True, {})[0] is None                 # per-stage instrumentation
        assert loops._fast_greedy(m.train(), False, True, None)[0] is None
    monkeypatch.setattr(S, 'fast_module', lambda: SimpleNamespace())            # a native module without the greedy driver
    assert loops._fast_greedy(TrackMPNN('2d', 3, 64, 0, 'diff').eval(), False, True, None)[0] is None


def _old_ladder(eligible, att, padded, N, cap, grad_on, x_grad, h_grad, any_pg, all_pg, inplace, native):
    """forward_dgraph and _forward_dgraph_padded as they stood, with every tensor and module replaced by the fact read
    from it: fast_module() -> native, the in-place flag + usable .grad buffers -> inplace.  Returns (path, padded width taken,
    node, grads, need_grad passed to the node | None on the staged path)."""
    small_ok = eligible and 0 < N <= DG_BIG_ROWS
    if padded and small_ok and not att:
        need_grad = grad_on and (any_pg or x_grad or h_grad)
        pgrad = grad_on and any_pg
        fast = native if cap == N else None
        if fast and pgrad and all_pg:
            return 'fused', True, 'native', 'sink', need_grad
        elif fast and not need_grad:
            return 'fused', True, 'native', 'none', False
        else:
            return 'fused', True, 'python', 'autograd' if need_grad else 'none', need_grad
    if padded or not small_ok:
        return 'staged', padded, '', '', None
    pgrad = grad_on and any_pg
    need_grad = grad_on and (pgrad or x_grad or h_grad)
    anchored = False
    if pgrad and inplace:
        anchored = True
    if anchored:
        fast = native if not att else None
        if fast and cap == N:
            return 'fused', False, 'native', 'inplace', need_grad
        else:
            return 'fused', False, 'python', 'inplace', need_grad
    elif not att and pgrad and native and cap == N and all_pg:
        return 'fused', False, 'native', 'sink', need_grad
    else:
        fast = native if not (need_grad or att) else None
        if fast and cap == N:
            return 'fused', False, 'native', 'none', False
        else:
            return 'fused', False, 'python', 'autograd' if need_grad else 'none', need_grad


def test_every_input_against_the_old_ladder():
    seen = set()
    for model in itertools.product((False, True), repeat=3):
        for N, dcap in itertools.product((0, 1, 64, 65535, 65536), (0, 7)):
            for flags in itertools.product((False, True), repeat=7):
                r = plan_small_route(*model, N, N + dcap, *flags)
                old = _old_ladder(*model, N, N + dcap, *flags)
                got = (r.path, r.padded, r.node, r.grads, r.need_grad if r.path == 'fused' else None)
                assert got == old, (model, N, dcap, flags)
                if r.path == 'staged':
                    grad_on, x_grad, h_grad, any_pg = flags[:4]
                    assert r.need_grad == (grad_on and (any_pg or x_grad or h_grad))
                seen.add(got)
    assert len(seen) == 2 + 4 + 6           # staged x padded ; fused padded ; fused true width


def test_route_is_frozen_and_takes_no_tensor():
    r = _route('h64')
    with pytest.raises(Exception):
        r.node = 'python'
    assert plan_small_route(1, 0, 0, 5, 5, 1, 0, 0, 1, 1, 0, 1) is _route('h64', N=9)      # (memoised by its booleans)
    with pytest.raises(Exception):
        plan_small_route(True, False, False, 5, 5, True, torch.ones(2), False, True, True, False, True)
